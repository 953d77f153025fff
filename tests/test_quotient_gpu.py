"""Quotient graphs and partition quality on the GPU (vgl_hip_quotient_plan_*, api.quotient_graph / partition_quality / modularity / condensation,
apps/bin/quotient_hip) against the restatement of the contract (tests/quotient_reference.py), against Graph.from_coo on the ascending list of distinct
coarse pairs, and composed with the library's other algorithms.  Every output is an integer and a function of the graph and the labels alone: plain
equality, the statistics included; the one float (modularity) is held to a bound derived from its formula."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import quotient_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("short", "wave", "table", "sorted")
COUNT_SLOTS = tuple("quot_count_" + k for k in CLASSES)
FILL_SLOTS = tuple("quot_fill_" + k for k in CLASSES)
SWITCHES = ("VGL_QUOT_SHORT", "VGL_QUOT_WAVE", "VGL_QUOT_TABLE", "VGL_QUOT_SORT_CAP_MB")
FOLLOW_SWITCHES = tuple("rows_%s_%s" % (k, d) for k in CLASSES for d in ("out", "in")) + ("sorted_keys_out", "sorted_keys_in", "sort_pieces_out",
                                                                                          "sort_pieces_in")


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def lib():
    from vectorgraphlibrary_amd import lib as L
    return L


def dev(ctx, a, dtype):
    return torch.tensor(np.asarray(a, dtype=dtype), device=ctx.device)


def graph(ctx, V, src, dst, renumber=None, with_incoming=True):
    return api().Graph.from_coo(ctx, V, dev(ctx, src, np.int32), dev(ctx, dst, np.int32), with_incoming=with_incoming, renumber=renumber)


def host(g):
    n = lambda t: None if t is None else t.cpu().numpy()
    return n(g.out_rowptr), n(g.out_adj), n(g.in_rowptr), n(g.in_adj)


def own(g, per_original):
    """a vertex array in ORIGINAL order -> the graph's own order"""
    a = np.asarray(per_original)
    return a if g.bwd is None else a[g.bwd.cpu().numpy()]


def tensors(q):
    return [t for t in (q.out_rowptr, q.out_adj, q.count, q.in_rowptr, q.in_adj, q.in_count, q.label_of, q.size, q.cluster_of) if t is not None]


def same_graph(a, b):
    return len(tensors(a)) == len(tensors(b)) and all(torch.equal(x, y) for x, y in zip(tensors(a), tensors(b)))


def set_switches(monkeypatch, short=None, wave=None, table=None, cap_mb=None):
    for name, val in zip(SWITCHES, (short, wave, table, cap_mb)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    d = lambda v, dflt: dflt if v is None else v
    return {"short": d(short, R.SHORT), "wave": d(wave, R.WAVE), "table": d(table, R.TABLE), "cap_mb": d(cap_mb, R.CAP_MB)}


def check_quot(ctx, g, labels, weights=None, self_loops=True, bounds=None, raw=False, from_coo=True, what=""):
    """api.quotient_graph(g, labels) against the restatement: both directions, counts, vertex maps, stats, and Graph.from_coo on the distinct pairs.
    labels: numpy, ORIGINAL order unless raw; weights: numpy int64 per stored outgoing entry."""
    A = api()
    rowptr, adj, in_rowptr, in_adj = host(g)
    lab_own = np.asarray(labels) if raw else own(g, labels)
    drop = not self_loops
    q = A.quotient_graph(g, torch.tensor(np.asarray(labels)), weights=None if weights is None else torch.tensor(weights), self_loops=self_loops, raw=raw)
    rp, ad, cnt = R.quotient_dir(rowptr, adj, lab_own, weights, drop)
    cluster_of, label_of, size = R.vertex_maps(lab_own)[:3]
    assert q.V == len(label_of) and q.fwd is None and q.bwd is None, what
    assert q.out_rowptr.dtype == torch.int64 and q.out_adj.dtype == torch.int32 and q.count.dtype == torch.int64, what
    assert np.array_equal(q.out_rowptr.cpu().numpy(), rp), what
    assert np.array_equal(q.out_adj.cpu().numpy(), ad), what
    assert np.array_equal(q.count.cpu().numpy(), cnt), what
    assert np.array_equal(q.label_of.cpu().numpy(), label_of) and np.array_equal(q.size.cpu().numpy(), size), what
    want_cluster = cluster_of if raw or g.fwd is None else cluster_of[g.fwd.cpu().numpy()]
    assert q.cluster_of.dtype == torch.int32 and np.array_equal(q.cluster_of.cpu().numpy(), want_cluster), what
    e_in = 0
    if in_rowptr is not None:
        irp, iad, icnt = R.quotient_dir(in_rowptr, in_adj, lab_own, None, drop)
        e_in = len(iad)
        if weights is not None:                                       # the transposition of the outgoing result; the counts follow its permutation
            irp2, iad2, perm = R.coo_to_csr(q.V, ad, R.rows_of(rp))
            assert np.array_equal(irp2, irp) and np.array_equal(iad2, iad), what
            icnt = cnt[perm]
        assert np.array_equal(q.in_rowptr.cpu().numpy(), irp) and np.array_equal(q.in_adj.cpu().numpy(), iad), what
        assert q.in_count.dtype == torch.int64 and np.array_equal(q.in_count.cpu().numpy(), icnt), what
    else:
        assert q.in_rowptr is None and q.in_adj is None and q.in_count is None, what
    b = bounds or {"short": R.SHORT, "wave": R.WAVE, "table": R.TABLE, "cap_mb": R.CAP_MB}
    ref = R.quotient_stats(rowptr, in_rowptr, lab_own, len(ad), e_in, **b)
    print("quotient", what, q.stats)
    assert q.stats == ref, (what, q.stats, ref)
    if from_coo:                                                      # bit-identical to the build over the ascending list of distinct coarse pairs
        f = A.Graph.from_coo(ctx, q.V, dev(ctx, R.rows_of(rp), np.int32), dev(ctx, ad, np.int32), with_incoming=in_rowptr is not None)
        assert torch.equal(f.out_rowptr, q.out_rowptr) and torch.equal(f.out_adj, q.out_adj), what
        if in_rowptr is not None:
            assert torch.equal(f.in_rowptr, q.in_rowptr) and torch.equal(f.in_adj, q.in_adj), what
    return q


# ---- 1. hand cases ----
@pytest.mark.parametrize("renumber", [None, "total"])
def test_hand_cases(ctx, renumber):
    for name, (V, src, dst) in R.hand_cases().items():
        g = graph(ctx, V, src, dst, renumber)
        w = (np.arange(g.E, dtype=np.int64) * 7 + 3) % 11
        for lname, labels in R.labelings(V).items():
            for self_loops in (True, False):
                check_quot(ctx, g, labels, None, self_loops, what="%s / %s / loops %s" % (name, lname, self_loops))
            check_quot(ctx, g, labels, w, True, what="%s / %s / weights" % (name, lname))
            check_quot(ctx, g, own(g, labels), None, True, raw=True, what="%s / %s / raw" % (name, lname))
        out_only = graph(ctx, V, src, dst, renumber, with_incoming=False)
        q = check_quot(ctx, out_only, R.labelings(V)["mod2"], what=name + " / out only")
        assert q.in_rowptr is None and q.stats["entries_in"] == 0


def test_a_cluster_of_isolated_vertices_is_an_empty_last_row(ctx):
    V, src, dst = R.hand_cases()["isolated"]                          # entries 1 <-> 3 only
    labels = np.array([0, 1, 0, 1, 8, 8])                             # cluster 2 = {4, 5}: isolated, the last row
    for renumber in (None, "total"):
        q = check_quot(ctx, graph(ctx, V, src, dst, renumber), labels, what="isolated cluster")
        assert q.out_rowptr.tolist() == [0, 0, 1, 1] and q.in_rowptr.tolist() == [0, 0, 1, 1] and q.count.tolist() == [2]


def test_members_through_the_c_call(ctx):
    L = lib()
    V, src, dst = R.hand_cases()["star"]
    g = graph(ctx, V, src, dst, "total")
    labels = own(g, np.array([4, 9, 4, 9, 9, 0, 4]))
    members, member_ptr = R.vertex_maps(labels)[3:]
    plan = C.c_void_p()
    L.check(ctx.L.vgl_hip_quotient_plan_create(ctx.h, g.h, C.c_void_p(dev(ctx, labels, np.int32).data_ptr()), 0, C.byref(plan)))
    try:
        m, mp = ctx.empty(V, torch.int32), ctx.empty(len(member_ptr), torch.int64)
        L.check(ctx.L.vgl_hip_quotient_plan_members(ctx.h, plan, C.c_void_p(m.data_ptr()), C.c_void_p(mp.data_ptr())))
        ctx.sync()
        assert np.array_equal(m.cpu().numpy(), members) and np.array_equal(mp.cpu().numpy(), member_ptr)
    finally:
        ctx.L.vgl_hip_quotient_plan_destroy(ctx.h, plan)


def test_failures(ctx):
    A, L = api(), lib()
    V, src, dst = R.hand_cases()["path"]
    g = graph(ctx, V, src, dst)
    out_only = graph(ctx, V, src, dst, with_incoming=False)
    with pytest.raises(L.VglHipError):
        A.quotient_graph(g, torch.tensor([0, 1, -1, 0, 1, 2]))
    with pytest.raises(L.VglHipError):
        A.quotient_graph(g, torch.tensor([0, 1, 2]))                  # a wrong length
    with pytest.raises(L.VglHipError):
        A.quotient_graph(g, torch.zeros(V, dtype=torch.int64), weights=torch.ones(3, dtype=torch.int64))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    plan = C.c_void_p()
    bad = dev(ctx, [0, 1, -5, 0, 1, 2], np.int32)
    assert ctx.L.vgl_hip_quotient_plan_create(ctx.h, g.h, ptr(bad), 0, C.byref(plan)) != 0      # the library's own check of the labels
    assert b"negative" in ctx.L.vgl_hip_last_error()
    assert ctx.L.vgl_hip_quotient_plan_create(ctx.h, g.h, None, 0, C.byref(plan)) != 0
    assert ctx.L.vgl_hip_quotient_plan_create(ctx.h, None, ptr(bad), 0, C.byref(plan)) != 0
    shard = g.shard(0, 3)
    assert ctx.L.vgl_hip_quotient_plan_create(ctx.h, shard.h, ptr(dev(ctx, [0] * V, np.int32)), 0, C.byref(plan)) != 0
    good = dev(ctx, [0, 0, 1, 1, 2, 2], np.int32)
    L.check(ctx.L.vgl_hip_quotient_plan_create(ctx.h, out_only.h, ptr(good), 0, C.byref(plan)))
    try:
        vc, eo, ei = C.c_int32(), C.c_int64(), C.c_int64()
        L.check(ctx.L.vgl_hip_quotient_plan_info(plan, C.byref(vc), C.byref(eo), C.byref(ei), None))
        assert (vc.value, eo.value, ei.value) == (3, 7, -1)
        rowptr, adj, count = torch.full((4,), -7, dtype=torch.int64, device=ctx.device), ctx.empty(7, torch.int32), ctx.empty(7, torch.int64)
        assert ctx.L.vgl_hip_quotient_plan_fill(ctx.h, plan, 1, None, ptr(rowptr), ptr(adj), ptr(count)) != 0      # no incoming CSR
        assert ctx.L.vgl_hip_quotient_plan_fill(ctx.h, plan, 2, None, ptr(rowptr), ptr(adj), ptr(count)) != 0
        assert ctx.L.vgl_hip_quotient_plan_fill(ctx.h, plan, 0, None, None, ptr(adj), ptr(count)) != 0
        assert ctx.L.vgl_hip_quotient_plan_fill(ctx.h, plan, 0, None, ptr(rowptr), None, ptr(count)) != 0
        assert ctx.L.vgl_hip_quotient_plan_fill(ctx.h, plan, 0, None, ptr(rowptr), ptr(adj), None) != 0
        ctx.sync()
        assert rowptr.tolist() == [-7] * 4                            # every failure happened before anything was written
        L.check(ctx.L.vgl_hip_quotient_plan_fill(ctx.h, plan, 0, None, ptr(rowptr), ptr(adj), ptr(count)))
        ctx.sync()
        assert rowptr.tolist() == [0, 2, 5, 7] and adj.tolist() == [0, 1, 0, 1, 2, 1, 2] and count.tolist() == [2, 1, 1, 2, 1, 1, 2]
    finally:
        ctx.L.vgl_hip_quotient_plan_destroy(ctx.h, plan)


# ---- 2. numbering independence ----
def test_numbering_independence(ctx):
    A = api()
    src, dst = (t.cpu().numpy() for t in ctx.gen_rmat(10, 8, 3))
    V = 1 << 10
    labels = torch.tensor(R.hashed_labels(V, 37, 5) * 11 + 2)
    plain, total = graph(ctx, V, src, dst, None), graph(ctx, V, src, dst, "total")
    for self_loops in (True, False):
        a, b = A.quotient_graph(plain, labels, self_loops=self_loops), A.quotient_graph(total, labels, self_loops=self_loops)
        assert same_graph(a, b) and a.in_rowptr is not None


# ---- 3. class boundaries ----
BOUND_ROWS = (2, 3, 8, 9, 16, 17)


def bounds_graph(ctx, equal):
    src = np.concatenate([np.full(m, i, dtype=np.int32) for i, m in enumerate(BOUND_ROWS)])
    dst = np.concatenate([np.full(m, 20, dtype=np.int32) if equal else 10 + np.arange(m, dtype=np.int32) for m in BOUND_ROWS])
    return graph(ctx, 64, src, dst)


def test_class_boundaries(ctx, monkeypatch):
    ident = np.arange(64) * 2
    for equal in (False, True):
        g = bounds_graph(ctx, equal)
        w = np.arange(g.E, dtype=np.int64) + 1
        first = [check_quot(ctx, g, ident, wt, what="bound rows, default switches") for wt in (None, w)]
        b = set_switches(monkeypatch, 2, 8, 16)
        second = [check_quot(ctx, g, ident, wt, bounds=b, what="bound rows, shrunk switches") for wt in (None, w)]
        set_switches(monkeypatch)
        assert [second[0].stats["rows_%s_out" % k] for k in CLASSES] == [1, 2, 2, 1]          # 2 | 3, 8 | 9, 16 | 17
        assert first[0].stats["rows_short_out"] == 6
        for x, y in zip(first, second):
            assert same_graph(x, y)
            assert {k: v for k, v in x.stats.items() if k not in FOLLOW_SWITCHES} == {k: v for k, v in y.stats.items() if k not in FOLLOW_SWITCHES}
        if equal:
            assert first[0].count.tolist() == list(BOUND_ROWS)


# ---- 4. the flat index over the members of a cluster ----
@pytest.mark.parametrize("renumber", [None, "total"])
def test_flat_index_over_members_in_every_class(ctx, monkeypatch, renumber):
    lens = [i % 4 for i in range(100)]
    lens[99] = 0                                                      # empty rows first and last
    V = 130
    src = np.concatenate([np.full(m, i, dtype=np.int32) for i, m in enumerate(lens)] + [np.arange(100, V, dtype=np.int32)])
    dst = np.concatenate([np.array([(i * 7 + j * 13) % V for j in range(m)], dtype=np.int32) for i, m in enumerate(lens)] + [np.arange(100, V, dtype=np.int32)[::-1]])
    labels = np.concatenate([np.full(100, 3), 10 + np.arange(30) % 6])
    g = graph(ctx, V, src, dst, renumber)
    w = (np.arange(g.E, dtype=np.int64) * 5) % 17 + 1
    volume = sum(lens)
    results = []
    for k, (short, wave, table) in enumerate(((256, 1024, 4096), (32, 1024, 4096), (32, 64, 4096), (32, 64, 100))):
        b = set_switches(monkeypatch, short, wave, table)
        assert R.class_rows([volume], short, wave, table)[k] == 1     # the cluster's row runs in class k
        for self_loops in (True, False):
            results.append(check_quot(ctx, g, labels, None, self_loops, bounds=b, what="100 members, class %s" % CLASSES[k]))
        results.append(check_quot(ctx, g, labels, w, True, bounds=b, what="100 members, weights, class %s" % CLASSES[k]))
    set_switches(monkeypatch)
    for i in range(3, len(results)):
        assert same_graph(results[i], results[i % 3])


# ---- 5. a full table ----
def full_row_graph(ctx, entries, copies):
    V = 1 << 16
    far = (np.arange(entries, dtype=np.int64) * (V // entries)).astype(np.int32)     # 0, V / entries, ...: equal modulo every smaller power of two
    dst = np.repeat(far, copies)[::-1].copy()
    return graph(ctx, V, np.zeros(len(dst), dtype=np.int32), dst, with_incoming=False)


def test_full_table_and_collisions(ctx, monkeypatch):
    ident = np.arange(1 << 16)
    b = set_switches(monkeypatch, 2, 8, 16)
    q = check_quot(ctx, full_row_graph(ctx, 16, 1), ident, bounds=b, from_coo=False, what="16 distinct far ends, table bound 16")
    assert q.stats["rows_table_out"] == 1 and q.out_adj.tolist() == [4096 * i for i in range(16)] and q.count.tolist() == [1] * 16
    q = check_quot(ctx, full_row_graph(ctx, 16, 3), ident, bounds=b, from_coo=False, what="16 far ends stored three times, table bound 16")
    assert q.stats["rows_sorted_out"] == 1 and q.out_adj.tolist() == [4096 * i for i in range(16)] and q.count.tolist() == [3] * 16      # 48 entries: past the bound
    b = set_switches(monkeypatch, 2, 8, 48)
    q = check_quot(ctx, full_row_graph(ctx, 16, 3), ident, bounds=b, from_coo=False, what="16 far ends stored three times, table bound 48")
    assert q.stats["rows_table_out"] == 1 and q.out_adj.tolist() == [4096 * i for i in range(16)] and q.count.tolist() == [3] * 16
    b = set_switches(monkeypatch)
    q = check_quot(ctx, full_row_graph(ctx, R.TABLE, 1), ident, from_coo=False, what="a row at the default table bound")
    assert q.stats["rows_table_out"] == 1 and q.stats["rows_sorted_out"] == 0 and q.E == R.TABLE
    q = check_quot(ctx, full_row_graph(ctx, R.WAVE, 1), ident, from_coo=False, what="a row at the default wave bound")
    assert q.stats["rows_wave_out"] == 1 and q.E == R.WAVE
    q = check_quot(ctx, full_row_graph(ctx, R.TABLE // 4, 4), ident, np.arange(R.TABLE, dtype=np.int64), from_coo=False, what="a full table of repeats, weights")
    assert q.stats["rows_table_out"] == 1 and q.E == R.TABLE // 4


# ---- 6. the sorted class in pieces ----
def test_sorted_class_in_pieces(ctx, monkeypatch):
    src, dst = (t.cpu().numpy() for t in ctx.gen_rmat(12, 16, 1))
    V = 1 << 12
    g = graph(ctx, V, src, dst)
    w = (np.arange(g.E, dtype=np.int64) * 3) % 1000
    four = R.hashed_labels(V, 4, 9)
    lopsided = (R.hashed_labels(V, 8, 9) == 0).astype(np.int64)       # cluster 0 holds seven vertices in eight: its row alone exceeds the cap
    for labels, what in ((four, "four clusters"), (lopsided, "one row above the cap")):
        b = set_switches(monkeypatch)
        whole = [check_quot(ctx, g, labels, wt, sl, what=what + ", no cap in reach") for wt, sl in ((None, True), (w, True), (None, False))]
        assert whole[0].stats["sort_pieces_out"] == 1 and whole[0].stats["rows_sorted_out"] == len(np.unique(labels))
        b = set_switches(monkeypatch, cap_mb=1)
        pieces = [check_quot(ctx, g, labels, wt, sl, bounds=b, what=what + ", cap 1 MB") for wt, sl in ((None, True), (w, True), (None, False))]
        set_switches(monkeypatch)
        assert pieces[0].stats["sort_pieces_out"] > 1 and pieces[0].stats["sort_pieces_in"] > 1
        assert all(same_graph(x, y) for x, y in zip(whole, pieces))
    vol = R.volumes(host(g)[0], lopsided)
    assert vol.max() > (1 << 20) // R.KEY_BYTES


# ---- 7. parity at scale ----
def scale_edges(ctx, kind):
    src, dst = ctx.gen_rmat(12, 16, 2) if kind == "rmat" else ctx.gen_uniform(14, 8, 2)
    return (1 << 12 if kind == "rmat" else 1 << 14), src.cpu().numpy(), dst.cpu().numpy()


@pytest.mark.parametrize("renumber", [None, "total"])
@pytest.mark.parametrize("kind", ["rmat", "uniform"])
def test_parity_at_scale(ctx, kind, renumber):
    A = api()
    V, src, dst = scale_edges(ctx, kind)
    g = graph(ctx, V, src, dst, renumber)
    sym = graph(ctx, V, np.concatenate([src, dst]), np.concatenate([dst, src]), renumber)
    labelings = {"hash K=%d" % K: R.hashed_labels(V, K, 4) for K in (1, 64, V // 4)}
    labelings["connected components"] = A.connected_components(sym, symmetric=True)[0].cpu().numpy()
    labelings["label propagation"] = A.label_propagation(g, max_iterations=5)[0].cpu().numpy()
    labelings["core numbers"] = A.core_numbers(g)[1]["core"].cpu().numpy()
    w = np.random.default_rng(3).integers(0, 1 << 20, size=g.E).astype(np.int64)
    for name, labels in labelings.items():
        check_quot(ctx, g, labels, what="%s %s / %s" % (kind, renumber, name))
        check_quot(ctx, g, labels, w, what="%s %s / %s / weights" % (kind, renumber, name))
    check_quot(ctx, g, labelings["hash K=64"], None, False, what="%s %s / no loops" % (kind, renumber))


# ---- 8. composition ----
def test_composition_on_the_device(ctx):
    A = api()
    src, dst = (t.cpu().numpy() for t in ctx.gen_rmat(11, 8, 6))
    V = 1 << 11
    g = graph(ctx, V, src, dst, "total")
    a = R.hashed_labels(V, 200, 1) * 3
    b = R.hashed_labels(200, 9, 2) + 50                               # by the label VALUE of the first step, so both sides name the same clusters
    first = A.quotient_graph(g, torch.tensor(a))
    b_of_coarse = b[(first.label_of.cpu().numpy() // 3)]
    for self_loops in (True, False):
        twice = A.quotient_graph(first, torch.tensor(b_of_coarse), weights=first.count, self_loops=self_loops)
        once = A.quotient_graph(g, torch.tensor(b[a // 3]), self_loops=self_loops)
        for x, y in ((twice.out_rowptr, once.out_rowptr), (twice.out_adj, once.out_adj), (twice.count, once.count), (twice.in_rowptr, once.in_rowptr),
                     (twice.in_adj, once.in_adj), (twice.in_count, once.in_count), (twice.label_of, once.label_of)):
            assert torch.equal(x, y)


# ---- 9. quality ----
def check_quality(ctx, g, labels, weights=None, what=""):
    A = api()
    rowptr, adj, _, _ = host(g)
    lab_own = own(g, labels)
    ref = R.quality(rowptr, adj, lab_own, weights)
    pq = A.partition_quality(g, torch.tensor(labels), weights=None if weights is None else torch.tensor(weights))
    for k in ("internal", "volume_out", "volume_in"):
        assert pq[k].dtype == torch.int64 and np.array_equal(pq[k].cpu().numpy(), ref[k]), (what, k)
    assert pq["total"] == ref["total"] and pq["cut"] == ref["cut"] and isinstance(pq["total"], int) and isinstance(pq["cut"], int), what
    assert int(pq["volume_out"].sum()) == int(pq["volume_in"].sum()) == pq["total"], what
    exact = R.modularity_fraction(rowptr, adj, lab_own, weights)
    err = abs(exact - R.Fraction(pq["modularity"]))
    print("modularity", what, pq["modularity"], "error", float(err), "bound", R.modularity_bound(len(ref["internal"])))
    assert err <= R.Fraction(R.modularity_bound(len(ref["internal"]))), what
    assert A.modularity(g, torch.tensor(labels), weights=None if weights is None else torch.tensor(weights)) == pq["modularity"], what
    assert pq["coverage"] == ((ref["total"] - ref["cut"]) / ref["total"] if ref["total"] else 1.0), what
    return pq


def test_quality(ctx):
    V, src, dst = scale_edges(ctx, "rmat")
    for renumber, with_in in ((None, True), ("total", True), (None, False)):
        g = graph(ctx, V, src, dst, renumber, with_incoming=with_in)
        w = np.random.default_rng(5).integers(0, 1 << 20, size=g.E).astype(np.int64)
        for K in (1, 7, V // 4):
            check_quality(ctx, g, R.hashed_labels(V, K, 8), what="rmat K=%d %s" % (K, renumber))
        check_quality(ctx, g, R.hashed_labels(V, 64, 8), w, what="rmat weights %s" % renumber)
    for n in (2, 5, 8):                                               # the closed forms
        V2, s2, d2 = R.two_cliques(n)
        for renumber in (None, "total"):
            g = graph(ctx, V2, s2, d2, renumber)
            pq = check_quality(ctx, g, (np.arange(V2) >= n).astype(np.int64), what="two K_%d" % n)
            assert abs(pq["modularity"] - 0.5) <= R.modularity_bound(2) and pq["cut"] == 0 and pq["coverage"] == 1.0
            one = check_quality(ctx, g, np.zeros(V2, dtype=np.int64), what="one cluster")
            assert abs(one["modularity"]) <= R.modularity_bound(1)
    empty = graph(ctx, 4, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert api().modularity(empty, torch.arange(4)) == 0.0


def test_closed_forms_of_the_quotient(ctx):
    rng = np.random.default_rng(7)
    V = 40
    pairs = np.unique(rng.integers(0, V, size=(300, 2)), axis=0)      # sorted unique COO
    g = graph(ctx, V, pairs[:, 0], pairs[:, 1])
    q = check_quot(ctx, g, np.arange(V) * 3 + 1, what="identity labels")
    assert torch.equal(q.out_rowptr, g.out_rowptr) and torch.equal(q.out_adj, g.out_adj) and torch.equal(q.in_adj, g.in_adj) and bool((q.count == 1).all())
    q = check_quot(ctx, g, np.full(V, 9), what="all equal")
    assert q.V == 1 and q.E == 1 and q.count.tolist() == [g.E]
    q = check_quot(ctx, g, np.full(V, 9), None, False, what="all equal, no loops")
    assert q.V == 1 and q.E == 0


# ---- 10. condensation ----
def test_condensation(ctx):
    A = api()
    src, dst = (t.cpu().numpy() for t in ctx.gen_rmat(10, 8, 4))
    V = 1 << 10
    for renumber in (None, "total"):
        g = graph(ctx, V, src, dst, renumber)
        comp = A.strongly_connected_components(g)[0].cpu().numpy()
        dag = A.condensation(g)
        assert dag.V == len(np.unique(comp))
        rows = torch.repeat_interleave(torch.arange(dag.V, device=ctx.device), dag.out_rowptr[1:] - dag.out_rowptr[:-1])
        assert not bool((dag.out_adj.long() == rows).any())
        assert len(np.unique(A.strongly_connected_components(dag)[0].cpu().numpy())) == dag.V      # acyclic
        assert int(dag.count.sum()) == int((comp[src] != comp[dst]).sum())
        assert np.array_equal(dag.label_of.cpu().numpy()[dag.cluster_of.cpu().numpy()], comp)
        check_quot(ctx, g, comp, None, False, what="condensation")


# ---- 11. the key bits of the two sorts at their edges ----
def test_sort_key_bits_at_their_edges(ctx, monkeypatch):
    # the vertex sort runs over the bits of the largest label: its top used bit at position 0 (none for the label 0 alone), 1, 15 and 30, with
    # labels one below the top value, whose low bits all count
    V = 300
    v = np.arange(V)
    src, dst = np.concatenate([v, [0, 7, 7, 150, 299]]), np.concatenate([(v * 11 + 1) % V, [299, 7, 8, 3, 0]])
    tops = {"0": 0, "0, 1": 1, "up to 2": 2, "up to 3": 3, "up to 32768": 1 << 15, "up to 2^30": 1 << 30}
    for renumber in (None, "total"):
        g = graph(ctx, V, src, dst, renumber)
        for name, top in tops.items():
            labels = np.array([top, max(top - 1, 0), top // 2, 0])[R.hashed_labels(V, 4, 5)]
            q = check_quot(ctx, g, labels, None, True, what="labels " + name)
            assert q.label_of.tolist() == sorted({top, max(top - 1, 0), top // 2, 0})
    # more than 2^16 clusters with every row in the sorted class: the 64-bit keys  c << 32 | c(w)  need 49 bits
    V = (1 << 16) + 4465
    v = np.arange(V)
    chord = v[v % 5 == 0]
    b = set_switches(monkeypatch, 0, 0, 0)
    q = check_quot(ctx, graph(ctx, V, np.concatenate([v, chord]), np.concatenate([(v + 1) % V, (chord * 7 + 3) % V])), V - 1 - v, bounds=b,
                   what="70001 clusters, sorted")
    set_switches(monkeypatch)
    assert q.V == V and q.stats["rows_sorted_out"] == V and q.stats["rows_short_out"] == 0


# ---- 12. determinism and hygiene ----
def test_determinism_and_launches(ctx, monkeypatch):
    A = api()
    V, src, dst = scale_edges(ctx, "rmat")
    g = graph(ctx, V, src, dst, "total")
    for labels, switches in ((R.hashed_labels(V, V // 4, 1), {}), (R.hashed_labels(V, 64, 1), {}), (R.hashed_labels(V, 3, 1), {}),
                             (R.hashed_labels(V, 64, 1), {"short": 0, "wave": 0, "table": 0}), (R.hashed_labels(V, 64, 1), {"short": 8, "wave": 64, "table": 512})):
        set_switches(monkeypatch, **switches)
        lab = torch.tensor(labels)
        ctx.timing(True)
        a = A.quotient_graph(g, lab)
        n = {k: ctx.timing_get(k)[0] for k in COUNT_SLOTS + FILL_SLOTS}
        ctx.timing(False)
        b = A.quotient_graph(g, lab)
        assert same_graph(a, b) and a.stats == b.stats
        for k in CLASSES[:3]:
            want = sum(a.stats["rows_%s_%s" % (k, d)] > 0 for d in ("out", "in"))
            assert n["quot_count_" + k] == want and n["quot_fill_" + k] == want, (k, n, a.stats)
        want = a.stats["sort_pieces_out"] + a.stats["sort_pieces_in"]
        assert n["quot_count_sorted"] == want and n["quot_fill_sorted"] == want, (n, a.stats)
    set_switches(monkeypatch)
    every = A.quotient_graph(g, torch.tensor(R.hashed_labels(V, 64, 1)))
    set_switches(monkeypatch, 0, 0, 0)
    forced = A.quotient_graph(g, torch.tensor(R.hashed_labels(V, 64, 1)))
    set_switches(monkeypatch)
    assert same_graph(every, forced) and forced.stats["rows_sorted_out"] == 64 and forced.stats["rows_table_out"] == 0


@pytest.mark.parametrize("extra", [[], ["-scc", "-noloops"], ["-cc"], ["-clusters", "3"]])
def test_app_check(tmp_path, extra):
    dump = str(tmp_path / "quotient.bin")
    cmd = [os.path.join(ROOT, "apps", "bin", "quotient_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-check", "-dump", dump] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "error count: 0" in out.stdout and "error count" not in out.stdout.replace("error count: 0", ""), out.stdout
    assert os.path.getsize(dump) % 24 == 0
