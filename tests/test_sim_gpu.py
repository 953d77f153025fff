"""Vertex similarity and link prediction on the GPU (vgl_hip_sim_pairs, vgl_hip_sim_topk, api.common_neighbors / similarity / adamic_adar /
resource_allocation / edge_similarity / link_prediction, apps/bin/sim_hip) against the restatement of the contract (tests/sim_reference.py), closed
forms and k-truss's triangle support.  Every integer output is a function of the graph alone: plain equality, the statistics included.  The one
floating-point output, the weighted sum, is held to a derived bound."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import sim_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_SLOTS = ("sim_pairs_short", "sim_pairs_wave", "sim_pairs_wg")
TOPK_SLOTS = ("sim_topk_small", "sim_topk_table", "sim_topk_global")
SHRUNK = {"VGL_SIM_SHORT": "2", "VGL_SIM_WAVE": "8", "VGL_SIM_TABLE_SMALL": "16", "VGL_SIM_TABLE": "64", "VGL_SIM_SCRATCH_MB": "1"}
PAIR_STATS = ("pairs", "pairs_short", "pairs_wave", "pairs_wg", "elements_examined", "common_total")
TOPK_STATS = ("queries", "two_paths_walked", "candidates_total", "filled")
API_METRICS = ("jaccard", "overlap", "sorensen")
_REF = {}


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def coo(ctx, src, dst):
    return (torch.tensor(np.asarray(src, dtype=np.int32), device=ctx.device), torch.tensor(np.asarray(dst, dtype=np.int32), device=ctx.device))


def launches(ctx, slots):
    return {n: ctx.timing_get(n)[0] for n in slots}


def numbers(st):
    return {k: v for k, v in st.items() if not torch.is_tensor(v)}


def check_pairs(g, G, u, v, what="", bounds=(32, 1024)):
    """common_neighbors and the three similarities of the pairs (ORIGINAL ids) against the restatement, the statistics included"""
    A = api()
    pairs = np.stack([np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)], axis=1)
    want = R.common(G, pairs[:, 0], pairs[:, 1])
    got = A.common_neighbors(g, pairs)
    assert got.dtype == torch.int32 and tuple(got.shape) == (pairs.shape[0],), what
    assert np.array_equal(got.cpu().numpy(), want), what
    du, dv = G["deg"][pairs[:, 0]], G["deg"][pairs[:, 1]]
    for metric in API_METRICS:
        s, st = A.similarity(g, torch.tensor(pairs), metric)
        assert s.dtype == torch.float64 and np.array_equal(st["common"].cpu().numpy(), want), (what, metric)
        assert np.array_equal(st["degree"].cpu().numpy(), G["deg"]), (what, metric)
        np.testing.assert_allclose(s.cpu().numpy(), R.score(metric, want, du, dv), rtol=4e-16, atol=0.0, err_msg=what + metric)
    ref = R.pair_stats(G, pairs[:, 0], pairs[:, 1], *bounds)
    print("pairs", what, numbers(st))
    for k in PAIR_STATS:
        assert st[k] == ref[k], (what, k, st[k], ref[k])
    assert st["algorithmic_bytes"] == R.pair_bytes(G, ref, degree_out=True), what
    return st


def check_topk(g, G, queries, k, metric, include=False, ref=None, what=""):
    """link_prediction of the queries (ORIGINAL ids; None: every vertex) against the restatement (ref: a restatement with at least k columns)"""
    A = api()
    ref = ref if ref is not None else R.topk(G, queries, k, metric, include)
    ids, com, score, st = A.link_prediction(g, k=k, metric=metric, vertices=None if queries is None else torch.tensor(np.asarray(queries)), include_neighbors=include)
    n = G["V"] if queries is None else len(queries)
    assert ids.dtype == com.dtype == torch.int32 and score.dtype == torch.float64 and tuple(ids.shape) == tuple(com.shape) == tuple(score.shape) == (n, k), what
    want_ids, want_c = ref["ids"][:, :k], ref["common"][:, :k]
    assert np.array_equal(ids.cpu().numpy(), want_ids), (what, metric, k, include)
    assert np.array_equal(com.cpu().numpy(), want_c), (what, metric, k, include)
    q = np.arange(G["V"]) if queries is None else np.asarray(queries, dtype=np.int64)
    held = want_ids >= 0
    want_s = np.where(held, R.score(metric, want_c, G["deg"][q][:, None], G["deg"][np.maximum(want_ids, 0)]), 0.0)
    np.testing.assert_allclose(score.cpu().numpy(), want_s, rtol=4e-16, atol=0.0, err_msg=what)
    assert st["queries"] == n and st["two_paths_walked"] == ref["two_paths_walked"] and st["candidates_total"] == ref["candidates_total"], (what, numbers(st))
    assert st["filled"] == int(held.sum()) and st["rows_small"] + st["rows_table"] + st["rows_global"] == n, (what, numbers(st))
    assert st["algorithmic_bytes"] == R.topk_bytes(ref, k), what
    return ids, com, st


# ---- 1. hand cases ----
@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
@pytest.mark.parametrize("renumber", [None, "total"])
def test_hand_cases(name, renumber, ctx):
    V, src, dst, G = R.hand_graph(name)
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber=renumber)
    a, b = np.meshgrid(np.arange(V), np.arange(V))                   # every ordered pair: u == v, adjacent, isolated and far pairs are all among them
    u, v = np.concatenate([a.ravel(), a.ravel()[:3]]), np.concatenate([b.ravel(), b.ravel()[:3]])      # ... and three of them once more
    check_pairs(g, G, u, v, what=name)
    for metric in ("common",) + API_METRICS:
        for include in (False, True):
            for k in (1, 3, 64):
                check_topk(g, G, None, k, metric if metric != "sorensen" else "jaccard", include, what=name)
                if metric == "sorensen":                              # ranks as Jaccard, scores as Sorensen
                    ids, com, score, _ = api().link_prediction(g, k=k, metric="sorensen", include_neighbors=include)
                    ref = R.topk(G, None, k, R.JACCARD, include)
                    assert np.array_equal(ids.cpu().numpy(), ref["ids"]) and np.array_equal(com.cpu().numpy(), ref["common"])
    score, st = api().edge_similarity(g, "jaccard")
    eu, ev, ec = R.edge_common(G)
    assert np.array_equal(st["edges"].cpu().numpy(), np.stack([eu, ev], axis=1)) and np.array_equal(st["common"].cpu().numpy(), ec), name
    g.close()


def test_hand_cases_closed_forms(ctx):
    A = api()
    V, src, dst, G = R.hand_graph("path5")
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    assert A.common_neighbors(g, [[0, 2], [1, 3], [0, 1], [0, 3], [2, 2], [0, 3]]).tolist() == [1, 1, 0, 0, 2, 0]      # distance 2, adjacent, distance 3, u == v, repeated
    ids, com, score, st = A.link_prediction(g, k=3, metric="jaccard")
    assert ids.tolist() == [[2, -1, -1], [3, -1, -1], [0, 4, -1], [1, -1, -1], [2, -1, -1]] and com.tolist() == [[1, 0, 0], [1, 0, 0], [1, 1, 0], [1, 0, 0], [1, 0, 0]]
    assert score[2].tolist() == [0.5, 0.5, 0.0] and st["filled"] == 6 and st["candidates_total"] == 6
    ids, com, _, _ = A.link_prediction(g, k=3, metric="common", vertices=[2, 2], include_neighbors=True)               # a repeated query is a row of its own
    assert ids.tolist() == [[0, 4, -1], [0, 4, -1]]
    g.close()
    V, src, dst, G = R.hand_graph("star")                             # hub 0, leaves 1 .. 6, vertex 7 isolated
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    s, st = A.similarity(g, [[1, 2], [3, 6], [7, 1], [7, 7], [0, 1]], "jaccard")
    assert s.tolist() == [1.0, 1.0, 0.0, 0.0, 0.0] and st["common"].tolist() == [1, 1, 0, 0, 0]
    ids, _, _, _ = A.link_prediction(g, k=64, vertices=[3, 0, 7])
    assert ids[0, :6].tolist() == [1, 2, 4, 5, 6, -1] and bool((ids[1:] == -1).all())
    g.close()
    V, src, dst, G = R.hand_graph("k6")
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    a, b = np.triu_indices(6, 1)
    assert bool((A.common_neighbors(g, np.stack([a, b], axis=1)) == 4).all())
    assert bool((A.link_prediction(g, k=5)[0] == -1).all())           # no 2-hop candidate that is not a neighbour
    assert A.link_prediction(g, k=5, include_neighbors=True)[0][0].tolist() == [1, 2, 3, 4, 5]
    g.close()
    V, src, dst, G = R.hand_graph("k34")
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber="total")
    s, st = A.similarity(g, [[0, 1], [3, 6], [0, 3]], "jaccard")
    assert st["common"].tolist() == [4, 3, 0] and s.tolist() == [1.0, 1.0, 0.0]
    assert A.link_prediction(g, k=4, vertices=[4, 0])[0].tolist() == [[3, 5, 6, -1], [1, 2, -1, -1]]       # ties by ORIGINAL id on the renumbered graph
    g.close()


def test_one_vertex_graph(ctx):
    A = api()
    g = A.Graph.from_coo(ctx, 1, *coo(ctx, [], []))
    assert A.common_neighbors(g, [[0, 0]]).tolist() == [0]
    s, st = A.similarity(g, [[0, 0]], "overlap")
    assert s.tolist() == [0.0] and st["degree"].tolist() == [0] and st["pairs_short"] == 1
    ids, com, score, st = A.link_prediction(g, k=2)
    assert ids.tolist() == [[-1, -1]] and com.tolist() == [[0, 0]] and score.tolist() == [[0.0, 0.0]] and st["rows_small"] == 1 and st["filled"] == 0
    assert A.common_neighbors(g, np.zeros((0, 2), dtype=np.int64)).numel() == 0
    g.close()


# ---- 2. generated graphs ----
def generated(ctx, kind, scale, ef, seed):
    """the graph (one more vertex than the generator's, so that the last one is isolated) and its reference results: built once, shared, left unchanged"""
    key = (kind, scale, ef, seed)
    if key not in _REF:
        src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
        src, dst = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
        V = (1 << scale) + 1
        G = R.simple_graph(V, src, dst)
        rng = np.random.default_rng(seed)
        u, v = rng.integers(0, V, 20000), rng.integers(0, V, 20000)
        queries = np.concatenate([rng.choice(V - 1, 254, replace=False), [int(np.argmax(G["deg"])), V - 1]])
        assert G["deg"][V - 1] == 0
        _REF[key] = {"V": V, "src": src, "dst": dst, "G": G, "u": u, "v": v, "queries": queries, "edges": R.edge_common(G),
                     "topk": {m: R.topk(G, queries, 64, m) for m in R.METRICS}}
    return _REF[key]


def variants(ctx, ref):
    A = api()
    V, s, d = ref["V"], *coo(ctx, ref["src"], ref["dst"])
    yield "directed", A.Graph.from_coo(ctx, V, s, d)
    yield "symmetrised", A.Graph.from_coo(ctx, V, torch.cat([s, d]), torch.cat([d, s]), with_incoming=False)
    yield "renumbered", A.Graph.from_coo(ctx, V, s, d, renumber="total")


@pytest.mark.parametrize("kind,scale", [("rmat", 10), ("rmat", 12), ("rmat", 14), ("uniform", 12)])
def test_generated_graphs(kind, scale, ctx):
    A = api()
    ref = generated(ctx, kind, scale, 16, 1)
    G = ref["G"]
    eu, ev, ec = ref["edges"]
    for what, g in variants(ctx, ref):
        what = "%s %d %s" % (kind, scale, what)
        check_pairs(g, G, ref["u"], ref["v"], what=what)
        for metric in ("common", "jaccard"):
            score, st = A.edge_similarity(g, metric)
            assert np.array_equal(st["edges"].cpu().numpy(), np.stack([eu, ev], axis=1)) and np.array_equal(st["common"].cpu().numpy(), ec), what
            np.testing.assert_allclose(score.cpu().numpy(), R.score(metric, ec, G["deg"][eu], G["deg"][ev]), rtol=4e-16, atol=0.0)
            assert st["pairs"] == eu.size and st["common_total"] == int(ec.sum()) and st["elements_examined"] == int(np.minimum(G["deg"][eu], G["deg"][ev]).sum()), what
        for metric in R.METRICS:
            for k in (1, 10, 64):
                check_topk(g, G, ref["queries"], k, metric, ref=ref["topk"][metric], what=what)      # the renumbered graph too: the same ORIGINAL ids
        g.close()


# ---- 3. an independent implementation ----
def test_edge_common_neighbours_are_the_triangle_support_of_ktruss(ctx):
    A = api()
    ref = generated(ctx, "rmat", 12, 16, 1)
    for what, g in variants(ctx, ref):
        _, st = A.edge_similarity(g, "common")
        _, tr = A.truss_numbers(g, support=True)
        assert torch.equal(st["edges"], tr["edges"]) and torch.equal(st["common"], tr["support"]), what
        assert st["common_total"] == 3 * tr["triangles"], what
        g.close()


# ---- 4. every class ----
def _with_a_star(ref, leaves=20):
    """the generated graph and a star of `leaves` leaves on new vertices: under the shrunk switches its vertices have 16 < work2 <= 64"""
    V = ref["V"]
    src = np.concatenate([ref["src"], np.full(leaves, V)])
    dst = np.concatenate([ref["dst"], V + 1 + np.arange(leaves)])
    return V + 1 + leaves, src, dst


def test_every_class_and_shrunk_switches(ctx, monkeypatch):
    A = api()
    ref = generated(ctx, "rmat", 12, 16, 1)
    V, src, dst = _with_a_star(ref)
    G = R.simple_graph(V, src, dst)
    s, d = coo(ctx, src, dst)
    g = A.Graph.from_coo(ctx, V, torch.cat([s, d]), torch.cat([d, s]), with_incoming=False)
    queries = np.concatenate([ref["queries"], [ref["V"], ref["V"] + 1, ref["V"] + 2]])      # ... and the star's hub and two of its leaves
    u, v = np.concatenate([ref["u"], [ref["V"]]]), np.concatenate([ref["v"], [ref["V"] + 3]])
    pairs = torch.tensor(np.stack([u, v], axis=1))
    weight = R.adamic_adar_weights(G["deg"])

    def run(bounds):
        ctx.timing(True)
        st = check_pairs(g, G, u, v, what="switches %s" % (bounds,), bounds=bounds)
        aa, _ = A.adamic_adar(g, pairs)
        n_pairs = launches(ctx, PAIR_SLOTS)
        ctx.timing(True)
        out = {m: check_topk(g, G, queries, 10, m, what="switches %s" % (bounds,)) for m in R.METRICS}
        n_topk = launches(ctx, TOPK_SLOTS)
        ctx.timing(False)
        return st, aa, out, n_pairs, n_topk

    st0, aa0, out0, p0, t0 = run((32, 1024))
    for k, val in SHRUNK.items():
        monkeypatch.setenv(k, val)
    st1, aa1, out1, p1, t1 = run((2, 8))
    print("launches under the default / shrunk switches", p0, p1, t0, t1)
    assert all(p1[k] > 0 for k in PAIR_SLOTS) and all(t1[k] > 0 for k in TOPK_SLOTS), (p1, t1)
    assert st1["pairs_short"] > 0 and st1["pairs_wave"] > 0 and st1["pairs_wg"] > 0, numbers(st1)
    assert torch.equal(st0["common"], st1["common"]) and st0["common_total"] == st1["common_total"] and st0["elements_examined"] == st1["elements_examined"]
    want, hits = R.weighted(G, u, v, weight)
    for aa in (aa0, aa1):                                            # another summation shape, the same bound
        assert bool((torch.tensor(np.abs(aa.cpu().numpy() - want) <= hits * 2.0 ** -52 * want)).all())
    for m in R.METRICS:
        (i0, c0, s0), (i1, c1, s1) = out0[m], out1[m]
        assert torch.equal(i0, i1) and torch.equal(c0, c1), m
        assert all(s0[k] == s1[k] for k in TOPK_STATS), (m, numbers(s0), numbers(s1))
        rows = R.topk_rows(G, queries, small=16, table=64)
        assert {k: s1[k] for k in rows} == rows and all(val > 0 for val in rows.values()), (numbers(s1), rows)
        assert {k: s0[k] for k in rows} == R.topk_rows(G, queries), numbers(s0)
        assert 1 <= s1["scratch_slots"] == min((1 << 20) // (8 * V), s1["rows_global"]) < s1["rows_global"], numbers(s1)      # slots are reused: the counters are cleared between rows
    monkeypatch.setenv("VGL_SIM_PAIR_CHUNK", "4096")                  # several list builds per call
    c = A.common_neighbors(g, pairs)
    assert torch.equal(c, st0["common"])
    aa2, _ = A.adamic_adar(g, pairs)
    assert torch.equal(aa2, aa1)                                      # the shape of the sum does not depend on the chunks
    g.close()


def test_double_star_reaches_the_global_class_under_the_default_switches(ctx):
    A = api()
    n = 6000
    leaves = 2 + np.arange(n)
    V, src, dst = n + 2, np.concatenate([np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)]), np.concatenate([leaves, leaves])
    G = R.simple_graph(V, src, dst)
    assert G["work2"][2] == 2 * n and G["work2"][0] == 2 * n
    queries = [2, 3, 11, 4000, 6001, 0, 1]
    for renumber in (None, "total"):
        g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber=renumber)
        ctx.timing(True)
        ids, com, st = check_topk(g, G, queries, 10, "jaccard", what="double star")
        t = launches(ctx, TOPK_SLOTS)
        ctx.timing(False)
        assert st["rows_global"] == len(queries) and st["rows_small"] == st["rows_table"] == 0 and t["sim_topk_global"] == 1 and t["sim_topk_small"] == t["sim_topk_table"] == 0, (numbers(st), t)
        assert st["scratch_slots"] == len(queries) and st["candidates_total"] == 5 * (n - 1) + 2
        assert ids[0].tolist() == list(range(3, 13)) and ids[1].tolist() == [2] + list(range(4, 13)) and ids[2].tolist() == list(range(2, 11)) + [12]
        assert bool((com[:5] == 2).all()) and ids[5].tolist() == [1] + [-1] * 9 and com[5].tolist() == [n] + [0] * 9 and ids[6, 0].item() == 0
        check_topk(g, G, queries, 64, "common", include=True, what="double star, neighbours too")
        g.close()


# ---- 5. the weighted sum ----
def test_weighted_sums_within_the_derived_bound_and_bit_identical(ctx):
    """|sum - fsum| <= hits 2^-52 S: for non-negative terms any summation order is within gamma_(hits - 1) S of the exact sum S (u = 2^-53), and fsum
    itself is within u S of it"""
    A = api()
    ref = generated(ctx, "rmat", 12, 16, 1)
    G = ref["G"]
    heavy = np.argsort(-G["deg"])[:24]                               # ... and the pairs of the heaviest vertices: long shorter rows, many hits
    hu, hv = np.meshgrid(heavy, heavy)
    u, v = np.concatenate([ref["u"][:5000], hu.ravel()]), np.concatenate([ref["v"][:5000], hv.ravel()])
    pairs = torch.tensor(np.stack([u, v], axis=1))
    wanted = {fn: R.weighted(G, u, v, weights(G["deg"])) for fn, weights in ((A.adamic_adar, R.adamic_adar_weights), (A.resource_allocation, R.resource_allocation_weights))}
    for what, g in variants(ctx, ref):
        for fn, (want, hits) in wanted.items():
            got, st = fn(g, pairs)
            again, _ = fn(g, pairs)
            assert got.dtype == torch.float64 and torch.equal(got, again), what          # bit-identical under the same switches
            assert np.array_equal(st["common"].cpu().numpy(), hits), what
            err = np.abs(got.cpu().numpy() - want)
            bound = hits * 2.0 ** -52 * want
            print(what, fn.__name__, "largest error / bound", float(np.max(err / np.maximum(bound, 1e-300))), "largest hits", int(hits.max()))
            assert bool((err <= bound).all()), (what, fn.__name__, float(err.max()))
            assert st["algorithmic_bytes"] == R.pair_bytes(G, R.pair_stats(G, u, v), weighted_out=True), what
        g.close()


# ---- 6. refusals ----
def test_refusals_write_nothing(ctx):
    A = api()
    ref = generated(ctx, "rmat", 10, 16, 1)
    V = ref["V"]
    g = A.Graph.from_coo(ctx, V, *coo(ctx, ref["src"], ref["dst"]))
    sh = g.shard(0, V // 2)
    L, E = ctx.L, A._l.VglHipError
    n = 64
    i32 = [torch.full((max(V, n * 65),), 0x5A5A5A5A, dtype=torch.int32, device=ctx.device) for _ in range(4)]
    f64 = torch.full((n,), -7.0, dtype=torch.float64, device=ctx.device)
    common, degree, ids, tk_common = [A._ptr(t) for t in i32]
    weighted = A._ptr(f64)
    u = torch.arange(n, dtype=torch.int32, device=ctx.device)
    bad = u.clone()
    bad[17] = V
    neg = u.clone()
    neg[3] = -1
    w = torch.ones(V, dtype=torch.float64, device=ctx.device)
    w_neg, w_nan, w_inf = w.clone(), w.clone(), w.clone()
    w_neg[5], w_nan[V - 1], w_inf[0] = -1e-300, float("nan"), float("inf")
    p = A._ptr
    for call in (sh.prepare_similarity, lambda: A.common_neighbors(sh, [[0, 1]]), lambda: A.link_prediction(sh, k=1, vertices=[0])):
        with pytest.raises(E, match="own all rows"):
            call()
    for handle, uu, vv, ww, c_out, w_out, match in (
            (sh.h, u, u, w, common, weighted, "own all rows"), (g.h, bad, u, w, common, weighted, r"outside \[0, V\)"), (g.h, u, neg, w, common, weighted, r"outside \[0, V\)"),
            (g.h, u, u, w_neg, common, weighted, "NaN, infinite or negative"), (g.h, u, u, w_nan, common, weighted, "NaN, infinite or negative"),
            (g.h, u, u, w_inf, None, weighted, "NaN, infinite or negative"), (g.h, u, u, None, common, weighted, "needs d_weight"), (g.h, u, u, w, None, None, "all outputs are NULL")):
        with pytest.raises(E, match=match):
            A._l.check(L.vgl_hip_sim_pairs(ctx.h, handle, p(uu), p(vv), n, p(ww), c_out, w_out, degree, None))
    with pytest.raises(E, match="n is negative"):
        A._l.check(L.vgl_hip_sim_pairs(ctx.h, g.h, p(u), p(u), -1, None, common, None, degree, None))
    for handle, q, nq, metric, k, match in (
            (sh.h, u, n, 1, 10, "own all rows"), (g.h, u, n, 1, 0, "k must be in"), (g.h, u, n, 1, 65, "k must be in"), (g.h, u, n, 3, 10, "unknown metric"),
            (g.h, bad, n, 1, 10, r"outside \[0, V\)"), (g.h, neg, n, 0, 10, r"outside \[0, V\)"), (g.h, u, -1, 1, 10, "n is negative"), (g.h, None, n, 1, 10, "n must equal V")):
        with pytest.raises(E, match=match):
            A._l.check(L.vgl_hip_sim_topk(ctx.h, handle, p(q) if q is not None else None, nq, metric, k, 0, None, ids, tk_common, None))
    with pytest.raises(E, match="d_ids must not be NULL"):
        A._l.check(L.vgl_hip_sim_topk(ctx.h, g.h, p(u), n, 1, 10, 0, None, None, tk_common, None))
    with pytest.raises(E, match="k must be in"):
        A.link_prediction(g, k=0)
    with pytest.raises(E, match="k must be in"):
        A.link_prediction(g, k=65)
    ctx.sync()
    assert all(bool((t == 0x5A5A5A5A).all()) for t in i32) and bool((f64 == -7.0).all())
    A._l.check(L.vgl_hip_sim_pairs(ctx.h, g.h, p(u), p(u), n, p(w), None, weighted, None, None))       # one output is enough; u == v: the weights of N(u)
    A._l.check(L.vgl_hip_sim_topk(ctx.h, g.h, p(u), n, 1, 64, 0, None, ids, None, None))                # d_common may be NULL
    ctx.sync()
    assert np.array_equal(f64.cpu().numpy(), ref["G"]["deg"][:n].astype(np.float64)) and bool((i32[0] == 0x5A5A5A5A).all()) and bool((i32[3] == 0x5A5A5A5A).all())
    assert np.array_equal(i32[2][:n * 64].cpu().numpy().reshape(n, 64), R.topk(ref["G"], np.arange(n), 64, R.JACCARD)["ids"]) and bool((i32[2][n * 64:] == 0x5A5A5A5A).all())
    for h in (sh, g):
        h.close()


# ---- 7. statistics and the cache ----
@pytest.mark.parametrize("first", ["sim", "kcore"])
def test_prepared_now_and_the_shared_cache(first, ctx):
    A = api()
    ref = generated(ctx, "rmat", 10, 16, 1)
    G = ref["G"]
    g = A.Graph.from_coo(ctx, ref["V"], *coo(ctx, ref["src"], ref["dst"]))
    pairs = torch.tensor(np.stack([ref["u"], ref["v"]], axis=1))
    if first == "kcore":                                              # the symmetric CSR is there already: the work2 stage is still this call's
        assert A.core_numbers(g)[1]["prepared_now"] == 1
    s0, a = A.similarity(g, pairs)
    s1, b = A.similarity(g, pairs)
    assert a["prepared_now"] == 1 and b["prepared_now"] == 0 and torch.equal(s0, s1) and torch.equal(a["common"], b["common"])
    assert np.array_equal(a["common"].cpu().numpy(), R.common(G, ref["u"], ref["v"]))
    assert all(a[k] == b[k] for k in PAIR_STATS + ("algorithmic_bytes",))
    assert A.link_prediction(g, k=3, vertices=[0, 1])[3]["prepared_now"] == 0
    assert A.core_numbers(g)[1]["prepared_now"] == 0                 # shared afterwards
    g.close()
    t = A.Graph.from_coo(ctx, ref["V"], *coo(ctx, ref["src"], ref["dst"]))
    if first == "kcore":
        t.prepare_kcore()
    ids0, com0, _, x = A.link_prediction(t, k=10, vertices=ref["queries"])
    ids1, com1, _, y = A.link_prediction(t, k=10, vertices=ref["queries"])
    assert x["prepared_now"] == 1 and y["prepared_now"] == 0 and torch.equal(ids0, ids1) and torch.equal(com0, com1)
    assert np.array_equal(ids0.cpu().numpy(), ref["topk"][R.JACCARD]["ids"][:, :10])
    assert all(x[k] == y[k] for k in TOPK_STATS + ("rows_small", "rows_table", "rows_global", "scratch_slots", "algorithmic_bytes"))
    t.close()
    p = A.Graph.from_coo(ctx, ref["V"], *coo(ctx, ref["src"], ref["dst"]))
    p.prepare_similarity()
    assert A.similarity(p, pairs)[1]["prepared_now"] == 0 and A.link_prediction(p, k=1, vertices=[0])[3]["prepared_now"] == 0
    p.close()


# ---- 8. the app ----
@pytest.mark.parametrize("mode", ["pairs", "edges", "topk"])
def test_sim_app(mode, tmp_path, ctx):
    dump = str(tmp_path / "sim.bin")
    extra = {"pairs": ["-pairs", "20000"], "edges": ["-pairs", "0"], "topk": ["-topk", "10", "-queries", "256"]}[mode]
    cmd = [os.path.join(ROOT, "apps", "bin", "sim_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-check", "-dump", dump] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "error count: 0" in out.stdout and "error count" not in out.stdout.replace("error count: 0", ""), out.stdout
    A = api()
    src, dst = ctx.gen_rmat(12, 16, 1)                               # what -gen generates: the app's default seed, the same generator
    g = A.Graph.from_coo(ctx, 1 << 12, src, dst)
    rec = np.fromfile(dump, np.int32).reshape(-1, 3)
    if mode == "topk":
        rec = rec.reshape(256, 10, 3)
        ids, com, _, _ = A.link_prediction(g, k=10, vertices=rec[:, 0, 0].copy())
        assert np.array_equal(ids.cpu().numpy(), rec[:, :, 1]) and np.array_equal(com.cpu().numpy(), rec[:, :, 2])
    else:
        assert rec.shape[0] == (20000 if mode == "pairs" else A.edge_similarity(g, "common")[1]["pairs"])
        assert np.array_equal(A.common_neighbors(g, rec[:, :2].copy()).cpu().numpy(), rec[:, 2])
    g.close()
