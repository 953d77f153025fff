"""Maximal independent set and maximal matching on the GPU (vgl_hip_mis_run, vgl_hip_matching_run, api.maximal_independent_set / maximal_matching /
vertex_cover, apps/bin/mis_hip) against the restatement of the contract (tests/mis_reference.py), closed forms and cross-checks on the device.
The answer is the lexicographically first set under the order: unique and an integer, so everything is exact equality, the statistics included."""
import os
import subprocess

import numpy as np
import pytest
import torch

import mis_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIS_SLOTS = ("mis_init", "mis_short", "mis_wave", "mis_wg", "mis_publish", "mis_finish")
MM_SLOTS = ("mm_init", "mm_best_short", "mm_best_wave", "mm_best_wg", "mm_match", "mm_publish")
MM_TENSORS = ("edges", "in_matching", "mate", "round")
_GRAPHS = {}


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def coo(ctx, src, dst):
    return (torch.tensor(np.asarray(src, dtype=np.int32), device=ctx.device), torch.tensor(np.asarray(dst, dtype=np.int32), device=ctx.device))


def graph_of(key, make):
    """(V, src, dst, the simple graph in ORIGINAL numbering) under `key`: built once, shared, left unchanged"""
    if key not in _GRAPHS:
        V, src, dst = make()
        src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        _GRAPHS[key] = (V, src, dst, R.simple_graph(V, src, dst))
    return _GRAPHS[key]


def generated(ctx, kind, scale, ef, seed):
    def make():
        src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
        return 1 << scale, src.cpu().numpy(), dst.cpu().numpy()
    return graph_of((kind, scale, ef, seed), make)


def u32(values):
    return torch.tensor(np.asarray(values).astype(np.int64))


def launches(ctx, slots):
    return {n: ctx.timing_get(n)[0] for n in slots}


def check_mis(g, G, vprio=None, seed=0, what=""):
    """one run (in_set and round, ORIGINAL order) against the rounds of the restatement; vprio: ORIGINAL order, free of ties when g is renumbered"""
    V = G["V"]
    ref = R.mis_rounds(G, vprio if vprio is not None else R.key(np.arange(V), seed))
    size, st = api().maximal_independent_set(g, priority=None if vprio is None else u32(vprio), seed=seed, rounds=True)
    print("mis", what, {k: v for k, v in st.items() if not torch.is_tensor(v)})
    assert st["in_set"].dtype == torch.bool and st["round"].dtype == torch.int32 and tuple(st["in_set"].shape) == tuple(st["round"].shape) == (V,), what
    assert np.array_equal(st["in_set"].cpu().numpy(), ref["in_set"]), what
    assert np.array_equal(st["round"].cpu().numpy(), ref["round"]), what
    for k in R.MIS_STATS:
        assert st[k] == ref[k], (what, k, st[k], ref[k])
    assert size == ref["set_size"], what
    assert st["algorithmic_bytes"] == R.algorithmic_bytes("mis", V, G["adj"].size, ref["live_total"], ref["entries_walked"], ref["rounds"]), what
    return st, ref


def own_graph(g, V, src, dst):
    """the simple graph in the numbering of g (its edge numbering is the library's)"""
    if g.fwd is None:
        return R.simple_graph(V, src, dst)
    fwd = g.fwd.cpu().numpy().astype(np.int64)
    return R.simple_graph(V, fwd[src], fwd[dst])


def check_matching(g, V, src, dst, eprio_of_original_edge=None, seed=0, what=""):
    """one raw run against the rounds of the restatement in the graph's own numbering, then the ORIGINAL-order view of the same result.
    eprio_of_original_edge: {(lo, hi) in ORIGINAL ids: priority}, or None for the default keys of the graph's own edge ids"""
    A = api()
    G = own_graph(g, V, src, dst)
    E = G["eu"].size
    bwd = g.bwd.cpu().numpy().astype(np.int64) if g.bwd is not None else np.arange(V)
    a, b = bwd[G["eu"]], bwd[G["ev"]]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    if eprio_of_original_edge is None:
        eprio, given = R.key(np.arange(E), seed), None
    else:
        eprio = np.array([eprio_of_original_edge[e] for e in zip(lo.tolist(), hi.tolist())], dtype=np.uint64)
        given = u32(eprio)
    ref = R.matching_rounds(G, eprio)
    m, raw = A.maximal_matching(g, edge_priority=given, seed=seed, raw=True)
    print("matching", what, {k: v for k, v in raw.items() if not torch.is_tensor(v)})
    assert raw["edges"].dtype == raw["mate"].dtype == raw["round"].dtype == torch.int32 and raw["in_matching"].dtype == torch.bool, what
    assert tuple(raw["edges"].shape) == (E, 2) and np.array_equal(raw["edges"].cpu().numpy(), np.stack([G["eu"], G["ev"]], axis=1)), what
    assert np.array_equal(raw["in_matching"].cpu().numpy(), ref["in_matching"]), what
    assert np.array_equal(raw["mate"].cpu().numpy(), ref["mate"]), what
    assert np.array_equal(raw["round"].cpu().numpy(), ref["round"]), what
    for k in R.MATCHING_STATS:
        assert raw[k] == ref[k], (what, k, raw[k], ref[k])
    assert m == ref["matched_edges"], what
    assert raw["algorithmic_bytes"] == R.algorithmic_bytes("matching", V, G["adj"].size, ref["live_total"], ref["entries_walked"], ref["rounds"]), what
    _, st = A.maximal_matching(g, edge_priority=given, seed=seed)
    order = np.lexsort((hi, lo))
    mate = np.full(V, -1, dtype=np.int64)
    mate[bwd] = np.where(ref["mate"] >= 0, bwd[np.maximum(ref["mate"], 0)], -1)
    rnd = np.zeros(V, dtype=np.int64)
    rnd[bwd] = ref["round"]
    assert np.array_equal(st["edges"].cpu().numpy(), np.stack([lo[order], hi[order]], axis=1)), what
    assert np.array_equal(st["in_matching"].cpu().numpy(), ref["in_matching"][order]), what
    assert np.array_equal(st["mate"].cpu().numpy(), mate) and np.array_equal(st["round"].cpu().numpy(), rnd), what
    cover = A.vertex_cover(g, edge_priority=given, seed=seed)
    assert cover.dtype == torch.bool and np.array_equal(cover.cpu().numpy(), mate >= 0), what
    return st, ref


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
@pytest.mark.parametrize("renumber", [None, "total"])
def test_hand_cases(name, renumber, ctx):
    V, stored, vprio, eprio, _, _ = R.HAND_CASES[name]
    G, vp, ep, in_set, mask = R.hand_case(name)
    src, dst = np.asarray([a for a, _ in stored], dtype=np.int64), np.asarray([b for _, b in stored], dtype=np.int64)
    if V == 0:                                                                   # a handle holds at least one vertex: the library's empty graph is one vertex without an edge
        with pytest.raises(api()._l.VglHipError, match="vertices_count must be positive"):
            api().Graph(ctx, 0, torch.zeros(1, dtype=torch.int64, device=ctx.device), torch.zeros(0, dtype=torch.int32, device=ctx.device))
        V, G, vp, in_set = 1, R.simple_graph(1, src, dst), np.zeros(1, dtype=np.uint64), np.ones(1, dtype=bool)
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber=renumber)
    st, _ = check_mis(g, G, vp, what=name)
    assert np.array_equal(st["in_set"].cpu().numpy(), in_set), name
    by_edge = {e: p for e, p in zip(zip(G["eu"].tolist(), G["ev"].tolist()), eprio)}
    st, _ = check_matching(g, V, src, dst, by_edge, what=name)
    assert np.array_equal(st["in_matching"].cpu().numpy(), mask), name
    g.close()


def _path(n):
    return n, np.arange(n - 1), np.arange(1, n)


def _star(n, hub):
    """vertices 0 .. n, `hub` among them"""
    leaves = np.array([v for v in range(n + 1) if v != hub])
    return n + 1, np.full(n, hub), leaves


def _complete(n):
    a, b = np.triu_indices(n, 1)
    return n, a, b


def _bipartite(n):
    a, b = np.meshgrid(np.arange(n), np.arange(n, 2 * n))
    return 2 * n, a.ravel(), b.ravel()


def test_path_64_in_id_order_and_reversed(ctx):
    """64 rounds of the independent set, 32 of the matching: one decision per round, the round of every vertex pinned"""
    V, src, dst, G = graph_of("path_64", lambda: _path(64))
    v = np.arange(64)
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    ctx.timing(True)
    st, ref = check_mis(g, G, v, what="path_64")
    n = launches(ctx, MIS_SLOTS)
    ctx.timing(False)
    assert st["rounds"] == 64 and st["set_size"] == 32 and st["live_total"] == 64 * 65 // 2
    assert np.array_equal(st["round"].cpu().numpy(), np.where(v % 2 == 0, 1, -1) * (v + 1))
    assert n["mis_short"] == 64 and n["mis_publish"] == 65 and n["mis_wave"] == n["mis_wg"] == 0 and n["mis_finish"] == 1, n
    st, ref = check_mis(g, G, 63 - v, what="path_64 reversed")
    assert st["rounds"] == 64 and np.array_equal(st["round"].cpu().numpy(), np.where(v % 2 == 1, 1, -1) * (64 - v))
    st, ref = check_matching(g, V, src, dst, {(i, i + 1): i for i in range(63)}, what="path_64")
    assert st["rounds"] == 32 and st["matched_edges"] == 32
    assert np.array_equal(st["mate"].cpu().numpy(), v ^ 1) and np.array_equal(st["round"].cpu().numpy(), v // 2 + 1)
    st, ref = check_matching(g, V, src, dst, {(i, i + 1): 62 - i for i in range(63)}, what="path_64 reversed")
    assert st["rounds"] == 32 and np.array_equal(st["mate"].cpu().numpy(), v ^ 1) and np.array_equal(st["round"].cpu().numpy(), (63 - v) // 2 + 1)
    g.close()


@pytest.mark.parametrize("hub_first", [True, False])
def test_star(hub_first, ctx):
    n, hub = 100, 37
    V, src, dst, G = graph_of("star_100", lambda: _star(n, hub))
    vprio = np.arange(V) + 1
    vprio[hub] = 0 if hub_first else V + 1
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    st, _ = check_mis(g, G, vprio, what="star")
    want = np.full(V, -2 if hub_first else 1)
    want[hub] = 1 if hub_first else -2
    assert st["rounds"] == 2 and st["set_size"] == (1 if hub_first else n) and np.array_equal(st["round"].cpu().numpy(), want)
    first = 5 if hub_first else 99
    st, _ = check_matching(g, V, src, dst, {(min(hub, w), max(hub, w)): (0 if w == first else 1 + w) for w in range(V) if w != hub}, what="star")
    assert st["rounds"] == 2 and st["matched_edges"] == 1 and int(st["mate"][hub]) == first and int(st["mate"][first]) == hub
    g.close()


def test_complete_and_complete_bipartite(ctx):
    A = api()
    V, src, dst, G = graph_of("k64", lambda: _complete(64))
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    st, _ = check_mis(g, G, np.arange(64), what="k64")
    assert st["set_size"] == 1 and st["rounds"] == 2 and bool(st["in_set"][0])
    st, _ = check_mis(g, G, None, seed=3, what="k64 default keys")
    assert st["set_size"] == 1 and st["rounds"] == 2
    st, _ = check_matching(g, V, src, dst, None, seed=3, what="k64")
    assert st["matched_edges"] == 32 and st["matched_vertices"] == 64
    g.close()
    V, src, dst, G = graph_of("k32_32", lambda: _bipartite(32))
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    st, _ = check_mis(g, G, np.arange(64), what="k32,32")
    assert st["set_size"] == 32 and st["rounds"] == 2 and bool(st["in_set"][:32].all())      # one side has no neighbour before it
    st, _ = check_matching(g, V, src, dst, None, seed=5, what="k32,32")
    assert st["matched_edges"] == 32
    g.close()


def test_all_equal_priorities_fall_to_the_ids(ctx):
    V, src, dst, G = generated(ctx, "rmat", 10, 4, 2)
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    st, _ = check_mis(g, G, np.full(V, 7), what="ties")
    assert bool(st["in_set"][0])                                                 # vertex 0 is the first of the order
    assert np.array_equal(st["in_set"].cpu().numpy(), R.greedy_mis_sequential(G, np.arange(V)))
    st, _ = check_matching(g, V, src, dst, {e: 7 for e in zip(G["eu"].tolist(), G["ev"].tolist())}, what="ties")
    assert np.array_equal(st["in_matching"].cpu().numpy(), R.greedy_matching_sequential(G, np.arange(G["eu"].size))[0])
    g.close()


def _star_on_a_ring():
    """hub 0 with the leaves 1 .. 2048; a ring of 4096 vertices; leaf 1 joined to the ring"""
    ring = 2049 + np.arange(4096)
    return 2049 + 4096, np.concatenate([np.zeros(2048, dtype=np.int64), ring, [1]]), np.concatenate([np.arange(1, 2049), 2049 + (np.arange(4096) + 1) % 4096, [2049]])


def _rows_at_the_bounds():
    """four hubs with rows of exactly 32, 33, 1024 and 1025 entries, their leaves on one ring (3 entries each), and a path of 10 vertices (1 or 2 entries)"""
    lens = (32, 33, 1024, 1025)
    src, dst, nxt = [], [], 4
    for h, n in enumerate(lens):
        src.append(np.full(n, h))
        dst.append(nxt + np.arange(n))
        nxt += n
    leaves = np.arange(4, nxt)
    src.append(leaves)
    dst.append(np.roll(leaves, -1))
    src.append(nxt + np.arange(9))
    dst.append(nxt + np.arange(1, 10))
    return nxt + 10, np.concatenate(src), np.concatenate(dst)


def test_the_hub_of_a_star_is_a_workgroup_row(ctx):
    V, src, dst, G = graph_of("star_ring", _star_on_a_ring)
    assert G["deg"][0] == 2048
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    ctx.timing(True)
    check_mis(g, G, None, seed=1, what="star on a ring")
    n = launches(ctx, MIS_SLOTS)
    check_matching(g, V, src, dst, None, seed=1, what="star on a ring")
    m = launches(ctx, MM_SLOTS)
    ctx.timing(False)
    assert n["mis_wg"] >= 1 and n["mis_wave"] == 0 and n["mis_short"] >= 1, n
    assert m["mm_best_wg"] >= 1 and m["mm_best_wave"] == 0 and m["mm_best_short"] >= 1, m
    vprio = np.arange(V) + 1                                                     # the hub last: it is a workgroup row in every round until it is decided
    vprio[0] = V + 1
    check_mis(g, G, vprio, what="star on a ring, the hub last")
    g.close()


SHRUNK = {"VGL_MIS_SHORT": "2", "VGL_MIS_WAVE": "8"}


def test_rows_at_the_class_bounds_and_shrunk_thresholds(ctx, monkeypatch):
    A = api()
    V, src, dst, G = graph_of("bounds", _rows_at_the_bounds)
    assert G["deg"][:4].tolist() == [32, 33, 1024, 1025]
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    hubs_last = np.arange(V) + 4
    hubs_last[:4] = V + 4 + np.arange(4)                                          # the four hubs are decided in the last round: every class works in every round
    ctx.timing(True)
    a0, _ = check_mis(g, G, hubs_last, what="default thresholds")
    b0, _ = check_mis(g, G, None, seed=2, what="default thresholds, default keys")
    n0 = launches(ctx, MIS_SLOTS)
    c0, _ = check_matching(g, V, src, dst, None, seed=2, what="default thresholds")
    m0 = launches(ctx, MM_SLOTS)
    assert n0["mis_wg"] >= 1 and n0["mis_wave"] >= 1 and n0["mis_short"] >= 1 and m0["mm_best_wg"] >= 1 and m0["mm_best_wave"] >= 1, (n0, m0)
    for k, v in SHRUNK.items():
        monkeypatch.setenv(k, v)
    ctx.timing(True)
    a1, _ = check_mis(g, G, hubs_last, what="shrunk thresholds")
    b1, _ = check_mis(g, G, None, seed=2, what="shrunk thresholds, default keys")
    n1 = launches(ctx, MIS_SLOTS)
    c1, _ = check_matching(g, V, src, dst, None, seed=2, what="shrunk thresholds")
    m1 = launches(ctx, MM_SLOTS)
    ctx.timing(False)
    print("launches under the default / shrunk thresholds", n0, n1, m0, m1)
    assert all(n1[k] > 0 for k in MIS_SLOTS) and all(m1[k] > 0 for k in MM_SLOTS), (n1, m1)
    for x, y in ((a0, a1), (b0, b1)):
        assert torch.equal(x["in_set"], y["in_set"]) and torch.equal(x["round"], y["round"])
        assert all(x[k] == y[k] for k in R.MIS_STATS + ("algorithmic_bytes",)), (x, y)
    assert all(torch.equal(c0[k], c1[k]) for k in MM_TENSORS)
    assert all(c0[k] == c1[k] for k in R.MATCHING_STATS + ("algorithmic_bytes",)), (c0, c1)
    g.close()


def test_item_counts_one_past_a_full_workgroup(ctx, monkeypatch):
    """33 short rows (a workgroup of 32 eight-lane teams and one more: 31 teams of the last workgroup have no row), 5 wave rows (4 + 1), 2 workgroup rows,
    row lengths on the bounds (tests/test_mis_cpu.py checks that the graph is that); the set, the matching, their rounds and statistics are the
    restatement's, under default keys and under priorities that decide the seven long rows last, so every class works until the last round"""
    V, src, dst, G = graph_of("team_edges", R.rows_at_the_team_edges)
    for k, v in zip(("VGL_MIS_SHORT", "VGL_MIS_WAVE"), R.TEAM_EDGE_BOUNDS):
        monkeypatch.setenv(k, str(v))
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    hubs_last = np.arange(V) + 1
    hubs_last[:7] = V + 1 + np.arange(7)
    ctx.timing(True)
    check_mis(g, G, None, seed=5, what="team edges, default keys")
    check_mis(g, G, hubs_last, what="team edges, the long rows last")
    n = launches(ctx, MIS_SLOTS)
    check_matching(g, V, src, dst, None, seed=5, what="team edges, default keys")
    edges = list(zip(G["eu"].tolist(), G["ev"].tolist()))
    check_matching(g, V, src, dst, {e: len(edges) - i for i, e in enumerate(edges)}, what="team edges, the edges in reverse")
    m = launches(ctx, MM_SLOTS)
    ctx.timing(False)
    print("launches", n, m)
    assert n["mis_short"] >= 1 and n["mis_wave"] >= 1 and n["mis_wg"] >= 1, n
    assert m["mm_best_short"] >= 1 and m["mm_best_wave"] >= 1 and m["mm_best_wg"] >= 1, m
    g.close()


@pytest.mark.parametrize("kind,scale,ef,seed", [("rmat", 12, 16, 1), ("uniform", 14, 8, 1)])
def test_generated_graphs(kind, scale, ef, seed, ctx):
    A = api()
    V, src, dst, G = generated(ctx, kind, scale, ef, seed)
    s, d = coo(ctx, src, dst)
    g = A.Graph.from_coo(ctx, V, s, d)
    a, _ = check_mis(g, G, None, seed=0, what="directed")
    check_matching(g, V, src, dst, None, seed=0, what="directed")
    g.close()
    r = A.Graph.from_coo(ctx, V, s, d, renumber="total")
    b, _ = check_mis(r, G, None, seed=0, what="renumbered")                      # the default keys are those of the ORIGINAL ids: the same set
    assert torch.equal(a["in_set"], b["in_set"]) and torch.equal(a["round"], b["round"])
    vprio = np.random.default_rng(seed).permutation(V)
    check_mis(r, G, vprio, what="renumbered, given priorities")
    check_matching(r, V, src, dst, None, seed=0, what="renumbered")
    own = own_graph(r, V, src, dst)                                              # raw: the keys of the graph's own ids
    _, raw = A.maximal_independent_set(r, rounds=True, raw=True)
    ref = R.mis_rounds(own, R.key(np.arange(V), 0))
    assert np.array_equal(raw["in_set"].cpu().numpy(), ref["in_set"]) and np.array_equal(raw["round"].cpu().numpy(), ref["round"])
    r.close()


def test_rmat_18_two_seeds(ctx):
    A = api()
    V, src, dst, G = generated(ctx, "rmat", 18, 8, 1)
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst), with_incoming=False)
    sets, matchings = [], []
    for seed in (0, 7):
        st, _ = check_mis(g, G, None, seed=seed, what="rmat 18 seed %d" % seed)
        sets.append(st["in_set"])
        st, _ = check_matching(g, V, src, dst, None, seed=seed, what="rmat 18 seed %d" % seed)
        matchings.append(st["in_matching"])
    assert not torch.equal(sets[0], sets[1]) and not torch.equal(matchings[0], matchings[1])
    g.close()


def test_two_runs_agree_and_prepare_is_cached(ctx):
    A = api()
    V, src, dst, G = generated(ctx, "rmat", 12, 16, 1)
    s, d = coo(ctx, src, dst)
    g = A.Graph.from_coo(ctx, V, s, d)
    _, a0 = A.maximal_independent_set(g, rounds=True)
    _, a1 = A.maximal_independent_set(g, rounds=True)
    assert a0["prepared_now"] == 1 and a1["prepared_now"] == 0
    assert torch.equal(a0["in_set"], a1["in_set"]) and torch.equal(a0["round"], a1["round"])
    assert all(a0[k] == a1[k] for k in R.MIS_STATS + ("algorithmic_bytes",)), (a0, a1)
    _, m0 = A.maximal_matching(g)
    _, m1 = A.maximal_matching(g)
    assert m0["prepared_now"] == 1 and m1["prepared_now"] == 0
    assert all(torch.equal(m0[k], m1[k]) for k in MM_TENSORS)
    assert all(m0[k] == m1[k] for k in R.MATCHING_STATS + ("algorithmic_bytes",)), (m0, m1)
    g.close()
    p = A.Graph.from_coo(ctx, V, s, d)
    p.prepare_mis()
    assert p.prepare_matching() == G["eu"].size
    assert A.maximal_independent_set(p)[1]["prepared_now"] == 0 and A.maximal_matching(p)[1]["prepared_now"] == 0
    p.close()


@pytest.mark.parametrize("first", ["ktruss", "bicc"])
def test_matching_reuses_the_edge_numbering(first, ctx):
    A = api()
    V, src, dst, G = generated(ctx, "rmat", 10, 16, 1)
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    other = A.truss_numbers(g)[1] if first == "ktruss" else A.biconnected_components(g)[1]
    _, mm = A.maximal_matching(g)
    assert other["prepared_now"] == 1 and mm["prepared_now"] == 0
    assert torch.equal(other["edges"], mm["edges"]) and other["undirected_edges"] == mm["undirected_edges"] == G["eu"].size
    g.close()


def test_cross_checks_on_the_device(ctx):
    A = api()
    V = 1 << 14
    src, dst = ctx.gen_rmat(14, 8, 5)
    g = A.Graph.from_coo(ctx, V, src, dst, renumber="total")
    rows = torch.repeat_interleave(torch.arange(V, device=ctx.device), g.out_rowptr[1:] - g.out_rowptr[:-1])
    cols = g.out_adj.long()
    off = rows != cols
    rows, cols = rows[off], cols[off]
    size, st = A.maximal_independent_set(g, seed=11, raw=True)
    s = st["in_set"]
    assert int(s.sum()) == size and not bool((s[rows] & s[cols]).any())          # no stored entry has both ends in the set
    seen = torch.zeros(V, dtype=torch.bool, device=ctx.device)
    seen[rows[s[cols]]] = True
    seen[cols[s[rows]]] = True
    assert bool((s | seen).all()) and not bool((s & seen).any())                 # every vertex outside the set has a neighbour in it
    m, mm = A.maximal_matching(g, seed=11, raw=True)
    mate = mm["mate"].long()
    matched = mate >= 0
    ids = torch.arange(V, device=ctx.device)
    assert bool((mate[mate[matched]] == ids[matched]).all())
    assert int(mm["in_matching"].sum()) * 2 == int(matched.sum()) == 2 * m == mm["matched_vertices"]
    assert bool((matched[rows] | matched[cols]).all())                           # every edge has a matched end
    e = mm["edges"][mm["in_matching"]].long()
    assert bool((mate[e[:, 0]] == e[:, 1]).all()) and bool((mate[e[:, 1]] == e[:, 0]).all())
    assert bool(((mm["round"] > 0) == matched).all())
    g.close()


def test_refusals_write_nothing(ctx):
    A = api()
    V, src, dst, G = generated(ctx, "rmat", 10, 4, 2)
    E = G["eu"].size
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    sh = g.shard(0, V // 2)
    for call in (lambda: A.maximal_independent_set(sh), lambda: A.maximal_matching(sh), sh.prepare_mis, sh.prepare_matching):
        with pytest.raises(A._l.VglHipError, match="own all rows"):
            call()
    i32 = [torch.full((max(E, V),), 0x5A5A5A5A, dtype=torch.int32, device=ctx.device) for _ in range(5)]
    u8 = [torch.full((max(E, V),), 0x5A, dtype=torch.uint8, device=ctx.device) for _ in range(2)]
    eu, ev, mate, rnd, mis_rnd = [A._ptr(t) for t in i32]
    mask, in_set = [A._ptr(t) for t in u8]
    L = ctx.L
    with pytest.raises(A._l.VglHipError, match="all outputs are NULL"):
        A._l.check(L.vgl_hip_mis_run(ctx.h, g.h, None, 0, None, None, None))
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        A._l.check(L.vgl_hip_mis_run(ctx.h, sh.h, None, 0, in_set, mis_rnd, None))
    with pytest.raises(A._l.VglHipError, match="all outputs are NULL"):
        A._l.check(L.vgl_hip_matching_run(ctx.h, g.h, None, 0, None, None, None, None, None, None))
    with pytest.raises(A._l.VglHipError, match="d_edge_u and d_edge_v"):
        A._l.check(L.vgl_hip_matching_run(ctx.h, g.h, None, 0, eu, None, mask, mate, rnd, None))
    with pytest.raises(A._l.VglHipError, match="d_edge_u and d_edge_v"):
        A._l.check(L.vgl_hip_matching_run(ctx.h, g.h, None, 0, None, ev, mask, mate, rnd, None))
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        A._l.check(L.vgl_hip_matching_run(ctx.h, sh.h, None, 0, eu, ev, mask, mate, rnd, None))
    ctx.sync()
    assert all(bool((t == 0x5A5A5A5A).all()) for t in i32) and all(bool((t == 0x5A).all()) for t in u8)
    A._l.check(L.vgl_hip_mis_run(ctx.h, g.h, None, 0, in_set, None, None))       # one output is enough
    A._l.check(L.vgl_hip_matching_run(ctx.h, g.h, None, 0, None, None, mask, None, None, None))
    ctx.sync()
    assert np.array_equal(u8[1][:V].cpu().numpy().astype(bool), R.mis_rounds(G, R.key(np.arange(V), 0))["in_set"]) and bool((u8[1][V:] == 0x5A).all())
    assert np.array_equal(u8[0][:E].cpu().numpy().astype(bool), R.matching_rounds(G, R.key(np.arange(E), 0))["in_matching"]) and bool((u8[0][E:] == 0x5A).all())
    for h in (sh, g):
        h.close()


@pytest.mark.parametrize("matching", [False, True])
def test_mis_app(matching, tmp_path, ctx):
    dump = str(tmp_path / "mis.bin")
    cmd = [os.path.join(ROOT, "apps", "bin", "mis_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-check", "-dump", dump] + (["-matching"] if matching else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "error count: 0" in out.stdout and "error count" not in out.stdout.replace("error count: 0", ""), out.stdout
    A = api()
    src, dst = ctx.gen_rmat(12, 16, 1)                                           # what -gen generates: the app's default seed, the same generator
    g = A.Graph.from_coo(ctx, 1 << 12, src, dst)
    if matching:
        _, st = A.maximal_matching(g, seed=1)
        want = torch.cat([st["edges"], st["in_matching"].to(torch.int32)[:, None]], dim=1).cpu().numpy()
    else:
        _, st = A.maximal_independent_set(g, seed=1, rounds=True)
        want = torch.stack([torch.arange(1 << 12, dtype=torch.int32, device=ctx.device), st["in_set"].to(torch.int32), st["round"]], dim=1).cpu().numpy()
    assert np.array_equal(np.fromfile(dump, np.int32).reshape(-1, 3), want)
    g.close()
