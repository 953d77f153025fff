"""Subgraph extraction, k-hop reach and neighbour sampling on the GPU (vgl_hip_subgraph_plan_*, vgl_hip_khop_run, vgl_hip_sample_neighbors,
api.induced_subgraph / edge_subgraph / k_hop / ego_graph / sample_neighbors / sample_blocks, apps/bin/subgraph_hip) against the restatement of the
contract (tests/subgraph_reference.py), against Graph.from_coo on the filtered edge list, and composed with the library's other algorithms.  Every
output is an integer and a function of the graph alone: plain equality, the statistics included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import subgraph_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_SLOTS = ("sub_count_short", "sub_count_wave", "sub_count_wg")
FILL_SLOTS = ("sub_fill_short", "sub_fill_wave", "sub_fill_wg")
SAMPLE_SLOTS = ("sample_short", "sample_wave", "sample_wg")
SHRUNK = {"VGL_SUB_SHORT": "2", "VGL_SUB_WAVE": "8", "VGL_SAMPLE_SHORT": "2", "VGL_SAMPLE_WAVE": "8"}
CLASS_STATS = ("rows_short_out", "rows_wave_out", "rows_wg_out", "rows_short_in", "rows_wave_in", "rows_wg_in", "rows_short", "rows_wave", "rows_wg")
_REF = {}


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def dev(ctx, a, dtype):
    return torch.tensor(np.asarray(a, dtype=dtype), device=ctx.device)


def coo(ctx, src, dst):
    return dev(ctx, src, np.int32), dev(ctx, dst, np.int32)


def host(g):
    """the graph's own CSR, both directions, as numpy"""
    n = lambda t: None if t is None else t.cpu().numpy()
    return n(g.out_rowptr), n(g.out_adj), n(g.in_rowptr), n(g.in_adj)


def launches(ctx, slots):
    return {n: ctx.timing_get(n)[0] for n in slots}


def same_stats(a, b, but=()):
    return {k: v for k, v in a.items() if k not in but} == {k: v for k, v in b.items() if k not in but}


def check_sub(ctx, g, sub, keep_own=None, entry=None, bounds=(32, 1024), from_coo=True, what=""):
    """a subgraph of g (keep_own: uint8 flags in g's own numbering, entry: flags per outgoing entry) against the restatement and against from_coo"""
    A = api()
    rowptr, adj, in_rowptr, in_adj = host(g)
    rp, ad, org, new_id, old_id = R.filter_rows(rowptr, adj, keep_own, entry)
    assert sub.V == len(old_id) and sub.fwd is None and sub.bwd is None, what
    assert sub.out_rowptr.dtype == torch.int64 and sub.out_adj.dtype == torch.int32 and sub.parent_ids.dtype == torch.int32, what
    assert np.array_equal(sub.out_rowptr.cpu().numpy(), rp) and np.array_equal(sub.out_adj.cpu().numpy(), ad), what
    want_parent = old_id if g.bwd is None else g.bwd.cpu().numpy()[old_id]
    assert np.array_equal(sub.parent_ids.cpu().numpy(), want_parent), what
    if sub.origin is not None:
        assert sub.origin.dtype == torch.int64 and np.array_equal(sub.origin.cpu().numpy(), org), what
        assert np.array_equal(adj[sub.origin.cpu().numpy()], old_id[sub.out_adj.cpu().numpy()]), what      # parent.adj[origin] == old_id[sub.adj]
    if in_rowptr is not None:
        if entry is None:
            irp, iad = R.filter_rows(in_rowptr, in_adj, keep_own)[:2]
        else:
            irp, iad = R.transpose(len(old_id), rp, ad)
        assert np.array_equal(sub.in_rowptr.cpu().numpy(), irp) and np.array_equal(sub.in_adj.cpu().numpy(), iad), what
    else:
        assert sub.in_rowptr is None and sub.in_adj is None, what
    ref = R.filter_stats(rowptr, adj, in_rowptr, in_adj, keep_own, entry, *bounds)
    print("subgraph", what, sub.stats)
    assert sub.stats == ref, (what, sub.stats, ref)
    if from_coo:                                                      # bit-identical to the build over the filtered list taken in CSR order
        src = R.rows_of(rp)
        f = A.Graph.from_coo(ctx, sub.V, *coo(ctx, src, ad), with_incoming=in_rowptr is not None)
        assert torch.equal(f.out_rowptr, sub.out_rowptr) and torch.equal(f.out_adj, sub.out_adj), what
        if in_rowptr is not None:
            assert torch.equal(f.in_rowptr, sub.in_rowptr) and torch.equal(f.in_adj, sub.in_adj), what
    return sub


def own_mask(g, mask_original):
    """uint8 flags in ORIGINAL vertex order -> the graph's own numbering"""
    m = np.asarray(mask_original).astype(np.uint8)
    return m if g.bwd is None else m[g.bwd.cpu().numpy()]


def check_sample(g, seeds_own, fanout, seed, direction="out", bounds=(32, 1024), what=""):
    A = api()
    rowptr, adj, in_rowptr, in_adj = host(g)
    rp_, ad_ = (rowptr, adj) if direction == "out" else (in_rowptr, in_adj)
    want_rp, want_ad, want_org, ref = R.sample(rp_, ad_, seeds_own, fanout, seed, *bounds)
    rp, ad, org, st = A.sample_neighbors(g, seeds_own, fanout, seed=seed, direction=direction, origin=True, raw=True)
    assert rp.dtype == torch.int64 and ad.dtype == torch.int32 and org.dtype == torch.int64, what
    assert np.array_equal(rp.cpu().numpy(), want_rp), what
    assert np.array_equal(ad.cpu().numpy(), want_ad) and np.array_equal(org.cpu().numpy(), want_org), what
    assert st == ref, (what, st, ref)
    return rp, ad, org, st


def check_khop(g, seeds_own, hops, direction="out", symmetric=False, what=""):
    A = api()
    rowptr, adj, in_rowptr, in_adj = host(g)
    want, ref = R.k_hop(rowptr, adj, in_rowptr, in_adj, seeds_own, hops, {"out": 0, "in": 1}[direction], symmetric)
    hop, st = A.k_hop(g, seeds_own, hops, direction=direction, symmetric=symmetric, raw=True, with_stats=True)
    assert hop.dtype == torch.int32 and np.array_equal(hop.cpu().numpy(), want), (what, hops, direction, symmetric)
    assert st == ref, (what, hops, direction, symmetric, st, ref)
    return hop


# ---- 1. hand cases ----
@pytest.mark.parametrize("name", sorted(R.hand_cases()))
@pytest.mark.parametrize("renumber", [None, "total"])
def test_hand_cases(name, renumber, ctx):
    A = api()
    V, src, dst = R.hand_cases()[name]
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber=renumber)
    one = np.zeros(V, dtype=bool)
    one[V - 1] = True
    for mask in (np.ones(V, dtype=bool), one, np.arange(V) % 2 == 0, np.arange(V) % 2 == 1):
        sub = A.induced_subgraph(g, torch.tensor(mask), origin=True)
        check_sub(ctx, g, sub, own_mask(g, mask), what="%s %s" % (name, mask.astype(int).tolist()))
        ids = A.induced_subgraph(g, np.nonzero(mask)[0].tolist())    # the same set as a list of ids
        assert torch.equal(ids.out_rowptr, sub.out_rowptr) and torch.equal(ids.out_adj, sub.out_adj) and torch.equal(ids.parent_ids, sub.parent_ids)
        if mask.all():                                                # the identity
            assert torch.equal(sub.out_rowptr, g.out_rowptr) and torch.equal(sub.out_adj, g.out_adj) and torch.equal(sub.in_adj, g.in_adj)
    with pytest.raises(A._l.VglHipError):
        A.induced_subgraph(g, torch.zeros(V, dtype=torch.bool))
    with pytest.raises(A._l.VglHipError):
        A.induced_subgraph(g, [])
    entry = (np.arange(g.E) % 2 == 0).astype(np.uint8)
    sub = A.edge_subgraph(g, torch.tensor(entry), origin=True)
    check_sub(ctx, g, sub, None, entry, what=name + " entries")
    assert sub.V == V
    out_only = A.induced_subgraph(g, torch.tensor(np.arange(V) % 2 == 0), with_incoming=False)
    assert out_only.in_rowptr is None
    rowptr, adj, in_rowptr, in_adj = host(g)
    for hops in (0, 1, 2, 10 ** 6):
        for direction, symmetric in (("out", False), ("in", False), ("out", True)):
            for seeds in ([0], [V - 1, 0, V - 1], []):
                check_khop(g, seeds, hops, direction, symmetric, what=name)
    for direction in ("out", "in"):
        for fanout in (1, 2, 3, 100):
            check_sample(g, list(range(V)) + [0, 0], fanout, 5, direction, what=name)


def test_hand_cases_closed_forms_and_original_ids(ctx):
    A = api()
    V, src, dst = R.hand_cases()["star"]
    for renumber in (None, "total"):
        g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber=renumber)
        sub = A.induced_subgraph(g, list(range(1, V)))                # the hub dropped: no edge is left
        assert sub.V == V - 1 and sub.E == 0 and sub.out_rowptr.tolist() == [0] * V and sorted(sub.parent_ids.tolist()) == list(range(1, V))
        sub = A.induced_subgraph(g, [0, 3, 5])                        # ORIGINAL ids in, ORIGINAL ids out
        ids = sub.parent_ids.tolist()
        hub = ids.index(0)
        assert sorted(ids) == [0, 3, 5] and sub.E == 4
        assert sorted(sub.out_adj[int(sub.out_rowptr[hub]):int(sub.out_rowptr[hub + 1])].tolist()) == [i for i in range(3) if i != hub]
        hop = A.k_hop(g, [3], 2)                                      # leaf -> hub -> the other leaves, in ORIGINAL order
        assert hop.tolist() == [1, 2, 2, 0, 2, 2, 2] and A.k_hop(g, [3], 1).tolist() == [1, -1, -1, 0, -1, -1, -1]
        ego = A.ego_graph(g, [3], 1)
        assert sorted(ego.parent_ids.tolist()) == [0, 3] and sorted(ego.hop.tolist()) == [0, 1] and ego.E == 2
        rp, ad, st = A.sample_neighbors(g, [0, 3], 100)               # every entry, as ORIGINAL ids
        assert rp.tolist() == [0, 6, 7] and sorted(ad[:6].tolist()) == list(range(1, 7)) and ad[6:].tolist() == [0] and st["sampled_total"] == 7
    n, m = 9, 4                                                       # K_n with m vertices kept is K_m
    s, d = R._both([(i, j) for i in range(n) for j in range(i + 1, n)])
    sub = A.induced_subgraph(A.Graph.from_coo(ctx, n, *coo(ctx, s, d)), [1, 4, 6, 8])
    assert sub.V == m and np.diff(sub.out_rowptr.cpu().numpy()).tolist() == [m - 1] * m and sub.parent_ids.tolist() == [1, 4, 6, 8]
    assert A.triangle_count(sub)[0] == 4


# ---- 2. parity at scale ----
def generated(ctx, kind, scale, ef, seed):
    key = (kind, scale, ef, seed)
    if key not in _REF:
        src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
        _REF[key] = {"V": 1 << scale, "src": src, "dst": dst}
    return _REF[key]


@pytest.mark.parametrize("kind", ["rmat", "uniform"])
@pytest.mark.parametrize("renumber", [None, "total"])
def test_parity_at_scale(kind, renumber, ctx):
    A = api()
    ref = generated(ctx, kind, 12, 16, 1)
    V = ref["V"]
    g = A.Graph.from_coo(ctx, V, ref["src"], ref["dst"], renumber=renumber)
    rng = np.random.default_rng(3)
    mask = rng.random(V) < 0.5
    sub = A.induced_subgraph(g, torch.tensor(mask), origin=True)
    check_sub(ctx, g, sub, own_mask(g, mask), what="%s %s vertex mask" % (kind, renumber))
    assert A.triangle_count(sub)[0] == R.triangle_count(sub.V, *R.filter_rows(*host(g)[:2], own_mask(g, mask))[:2])
    entry = (rng.random(g.E) < 0.5).astype(np.uint8)
    sub = A.edge_subgraph(g, torch.tensor(entry), origin=True)
    check_sub(ctx, g, sub, None, entry, what="%s %s entry mask" % (kind, renumber))
    out_only = A.Graph.from_coo(ctx, V, ref["src"], ref["dst"], with_incoming=False, renumber=renumber)
    check_sub(ctx, out_only, A.induced_subgraph(out_only, torch.tensor(mask)), own_mask(out_only, mask), what="no incoming CSR")
    seeds = rng.integers(0, V, 300)
    for fanout, seed in ((1, 0), (5, 0), (25, 7)):
        for direction in ("out", "in"):
            check_sample(g, seeds, fanout, seed, direction, what=kind)
    for hops in (0, 1, 2, 10 ** 6):
        check_khop(g, seeds[:5], hops, "out", what=kind)
    check_khop(g, seeds[:5], 2, "in", what=kind)
    check_khop(g, seeds[:5], 3, "out", True, what=kind)


# ---- 3. the ordered compaction at its edges ----
BOUND_ROWS = (32, 33, 1024, 1025, 5000)         # vertex r has BOUND_ROWS[r] outgoing entries, entry j goes to vertex 10 + j


def bounds_graph(ctx):
    if "bounds" not in _REF:
        src = np.concatenate([np.full(n, r, dtype=np.int32) for r, n in enumerate(BOUND_ROWS)])
        dst = np.concatenate([10 + np.arange(n, dtype=np.int32) for n in BOUND_ROWS])
        V = 10 + max(BOUND_ROWS)
        _REF["bounds"] = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    return _REF["bounds"]


def keep_patterns():
    """which entries j of every row survive"""
    n = max(BOUND_ROWS)
    j = np.arange(n)
    yield "lane 63 and lane 0 of neighbouring chunks", np.isin(j, [7, 8, 63, 64, 255, 256, 1023, 1024, 4095, 4096])
    yield "the last wavefront only", (j >= 192) & (j < 256)
    yield "none in whole chunks", ((j >= 512) & (j < 600)) | (j >= 4990)
    yield "all", np.ones(n, dtype=bool)
    yield "alternating", j % 2 == 1
    yield "the last entry", j == n - 1


def test_ordered_compaction_at_the_class_bounds_and_shrunk_switches(ctx, monkeypatch):
    A = api()
    g = bounds_graph(ctx)
    V = g.V

    def run(bounds):
        out = []
        for what, pattern in keep_patterns():
            keep = np.zeros(V, dtype=np.uint8)
            keep[:10] = 1
            keep[10:] = pattern
            ctx.timing(True)
            sub = check_sub(ctx, g, A.induced_subgraph(g, torch.tensor(keep.astype(bool)), origin=True), keep, bounds=bounds, what=what)
            n = launches(ctx, COUNT_SLOTS + FILL_SLOTS)
            ctx.timing(False)
            entry = np.concatenate([pattern[:m] for m in BOUND_ROWS]).astype(np.uint8)
            esub = check_sub(ctx, g, A.edge_subgraph(g, torch.tensor(entry), origin=True), None, entry, bounds=bounds, what=what + " (entries)")
            out.append((sub, esub, n))
        return out

    first = run((32, 1024))
    for _, _, n in first:                                             # rows of 32 | 33, 1024 | 1025, 5000: every class, both passes, both directions
        assert all(n[k] >= 1 for k in COUNT_SLOTS + FILL_SLOTS[:1]), n
    assert all(first[3][2][k] >= 1 for k in FILL_SLOTS), first[3][2]
    for k, val in SHRUNK.items():
        monkeypatch.setenv(k, val)
    second = run((2, 8))
    for (a, ea, _), (b, eb, _) in zip(first, second):
        for x, y in ((a, b), (ea, eb)):
            assert torch.equal(x.out_rowptr, y.out_rowptr) and torch.equal(x.out_adj, y.out_adj) and torch.equal(x.origin, y.origin)
            assert torch.equal(x.in_rowptr, y.in_rowptr) and torch.equal(x.in_adj, y.in_adj) and torch.equal(x.parent_ids, y.parent_ids)
            assert same_stats(x.stats, y.stats, but=CLASS_STATS)      # the rows per class are what the switches move; each run equals the restatement's


def test_sampling_at_the_class_bounds_and_shrunk_switches(ctx, monkeypatch):
    g = bounds_graph(ctx)
    seeds = [0, 1, 2, 3, 4, 4, 0, 9, 10]                              # repeats; 9 has no entry; 10 has five incoming ones
    fanouts = (1, 5, 32, 33, 1024, 1025, 2000, 5000, 5001)            # 1, 5, 2000, and deg / deg + 1 of every row

    def run(bounds):
        out = []
        for seed in (0, 12345):
            for fanout in fanouts:
                ctx.timing(True)
                out.append(check_sample(g, seeds, fanout, seed, "out", bounds, what="bounds graph")[:3])
                n = launches(ctx, SAMPLE_SLOTS)
                ctx.timing(False)
                assert bounds != (32, 1024) or all(n[k] == 1 for k in SAMPLE_SLOTS), n      # rows of 32 | 33, 1024 | 1025, 5000: every class
            for fanout in (1, 4, 5, 6):
                out.append(check_sample(g, [10, 41, 42, 43, 1033, 1034, 1035, 5009, 0], fanout, seed, "in", bounds, what="bounds graph, incoming")[:3])
        return out

    first = run((32, 1024))
    for k, val in SHRUNK.items():
        monkeypatch.setenv(k, val)
    second = run((2, 8))
    for a, b in zip(first, second):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_sample_blocks(ctx):
    A = api()
    ref = generated(ctx, "rmat", 12, 16, 1)
    g = A.Graph.from_coo(ctx, ref["V"], ref["src"], ref["dst"], renumber="total")
    rowptr, adj, _, _ = host(g)
    seeds = [5, 17, 5, 900]
    blocks = A.sample_blocks(g, seeds, [5, 3, 2], seed=11, raw=True)
    want = R.sample_blocks(rowptr, adj, seeds, [5, 3, 2], 11)
    assert len(blocks) == len(want) == 3
    for b, (front, rp, ad) in zip(blocks, want):
        assert np.array_equal(b["seeds"].cpu().numpy(), front) and np.array_equal(b["rowptr"].cpu().numpy(), rp) and np.array_equal(b["adj"].cpu().numpy(), ad)
    bwd = g.bwd.cpu().numpy()                                         # ORIGINAL ids in and out: the same blocks, relabelled
    orig = A.sample_blocks(g, bwd[seeds].tolist(), [5, 3, 2], seed=11)
    for b, (front, rp, ad) in zip(orig, want):
        assert np.array_equal(b["seeds"].cpu().numpy(), bwd[front]) and np.array_equal(b["adj"].cpu().numpy(), bwd[ad])


# ---- 4. composition with the other algorithms ----
def test_composition(ctx):
    A = api()
    ref = generated(ctx, "rmat", 12, 16, 1)
    V = ref["V"]
    g = A.Graph.from_coo(ctx, V, ref["src"], ref["dst"], renumber="total")
    core = A.core_numbers(g)[1]["core"]
    k = 8
    inside = A.k_core(g, k)
    assert int(inside.sum()) > 0
    sub = A.induced_subgraph(g, inside)
    assert torch.equal(A.core_numbers(sub)[1]["core"], core[sub.parent_ids.long()])      # the cores >= k live inside the k-core
    seed = int(torch.argmax(g.to_original((g.out_rowptr[1:] - g.out_rowptr[:-1]).to(torch.int32))))
    levels, _ = A.bfs(g, seed)
    for h in (1, 2):
        ego = A.ego_graph(g, [seed], h)
        at = ego.parent_ids.tolist().index(seed)
        inner, _ = A.bfs(ego, at)
        base = int(levels[seed])                                      # bfs() numbers the source's level as the reference does
        assert torch.equal(inner, levels[ego.parent_ids.long()]) and int(inner.max()) <= base + h and int(inner.min()) == base
        assert torch.equal(ego.hop, inner - base) and ego.V == int(((levels >= base) & (levels <= base + h)).sum())
    mask = np.random.default_rng(5).random(V) < 0.3
    sub = A.induced_subgraph(g, torch.tensor(mask))
    assert A.triangle_count(sub)[0] == R.triangle_count(sub.V, *R.filter_rows(*host(g)[:2], own_mask(g, mask))[:2])


# ---- 5. k-hop on a long path: many levels with tiny frontiers ----
def test_k_hop_on_a_path(ctx):
    A = api()
    n = 3000
    g = A.Graph.from_coo(ctx, n, *coo(ctx, np.arange(n - 1), np.arange(1, n)))      # 0 -> 1 -> ... -> n - 1
    for hops in (0, 1, 2, 10 ** 6):
        check_khop(g, [0], hops, "out", what="path")
        check_khop(g, [n - 1, n - 1], hops, "in", what="path")
    hop = check_khop(g, [1500, 7, 1500], 10 ** 6, "out", True, what="path")
    assert int(hop.max()) == 1499 and int(hop.min()) == 0
    assert check_khop(g, [0], 10 ** 6, "out").tolist() == list(range(n))
    assert check_khop(g, [0], 10 ** 6, "in").tolist() == [0] + [-1] * (n - 1)


# ---- 6. refusals write nothing ----
def test_refusals_write_nothing(ctx):
    A = api()
    L = ctx.L
    ref = generated(ctx, "rmat", 10, 16, 1)
    V = ref["V"]
    g = A.Graph.from_coo(ctx, V, ref["src"], ref["dst"])
    out_only = A.Graph.from_coo(ctx, V, ref["src"], ref["dst"], with_incoming=False)
    shard = g.shard(0, V // 2)
    p = lambda t: C.c_void_p(t.data_ptr())
    keep = torch.ones(V, dtype=torch.uint8, device=ctx.device)
    seeds = dev(ctx, [1, 2, 3], np.int32)
    bad = dev(ctx, [1, V, 3], np.int32)
    neg = dev(ctx, [1, -1, 3], np.int32)

    plan = C.c_void_p()
    for graph, kv in ((g, None), (shard, keep)):                      # both masks NULL; a sharded handle
        assert L.vgl_hip_subgraph_plan_create(ctx.h, graph.h, p(kv) if kv is not None else None, None, C.byref(plan)) != 0 and plan.value is None
    assert L.vgl_hip_subgraph_plan_create(ctx.h, None, p(keep), None, C.byref(plan)) != 0 and plan.value is None
    rp = torch.full((V + 1,), 7, dtype=torch.int64, device=ctx.device)
    ad = torch.full((g.E,), 7, dtype=torch.int32, device=ctx.device)
    entry = torch.ones(g.E, dtype=torch.uint8, device=ctx.device)
    for graph, ke in ((g, entry), (out_only, None)):                  # direction 1 with an entry mask; without an incoming CSR
        assert L.vgl_hip_subgraph_plan_create(ctx.h, graph.h, p(keep), p(ke) if ke is not None else None, C.byref(plan)) == 0
        ei = C.c_int64()
        assert L.vgl_hip_subgraph_plan_info(plan, None, None, C.byref(ei), None) == 0 and ei.value == -1
        assert L.vgl_hip_subgraph_plan_fill(ctx.h, plan, 1, p(rp), p(ad), None) != 0
        assert L.vgl_hip_subgraph_plan_fill(ctx.h, plan, 2, p(rp), p(ad), None) != 0
        assert L.vgl_hip_subgraph_plan_fill(ctx.h, plan, 0, None, p(ad), None) != 0
        assert L.vgl_hip_subgraph_plan_destroy(ctx.h, plan) == 0
    none = torch.zeros(V, dtype=torch.uint8, device=ctx.device)      # V' = 0 is a valid plan whose fill writes nothing
    assert L.vgl_hip_subgraph_plan_create(ctx.h, g.h, p(none), None, C.byref(plan)) == 0
    vk, eo = C.c_int32(-1), C.c_int64(-1)
    assert L.vgl_hip_subgraph_plan_info(plan, C.byref(vk), C.byref(eo), None, None) == 0 and vk.value == 0 and eo.value == 0
    assert L.vgl_hip_subgraph_plan_fill(ctx.h, plan, 0, p(rp), p(ad), None) == 0 and L.vgl_hip_subgraph_plan_fill(ctx.h, plan, 1, p(rp), p(ad), None) == 0
    assert L.vgl_hip_subgraph_plan_destroy(ctx.h, plan) == 0
    ctx.sync()
    assert int((rp != 7).sum()) == 0 and int((ad != 7).sum()) == 0

    hop = torch.full((V,), 7, dtype=torch.int32, device=ctx.device)
    khop = lambda graph, s, n, hops, d, sym: L.vgl_hip_khop_run(ctx.h, graph.h, p(s), n, hops, d, sym, p(hop), None)
    assert khop(g, bad, 3, 2, 0, 0) != 0 and b"seed" in L.vgl_hip_last_error()
    assert khop(g, neg, 3, 2, 0, 0) != 0
    assert khop(g, seeds, 3, -1, 0, 0) != 0 and b"hops" in L.vgl_hip_last_error()
    assert khop(g, seeds, -1, 1, 0, 0) != 0
    assert khop(g, seeds, 3, 1, 2, 0) != 0
    assert khop(out_only, seeds, 3, 1, 0, 1) != 0 and b"incoming" in L.vgl_hip_last_error()
    assert khop(out_only, seeds, 3, 1, 1, 0) != 0
    assert khop(shard, seeds, 3, 1, 0, 0) != 0
    assert L.vgl_hip_khop_run(ctx.h, g.h, p(seeds), 3, 1, 0, 0, None, None) != 0
    ctx.sync()
    assert int((hop != 7).sum()) == 0
    assert khop(g, seeds, 0, 5, 0, 0) == 0 and int((hop != -1).sum()) == 0      # no seeds: a success, nothing is reached

    srp = torch.full((4,), 7, dtype=torch.int64, device=ctx.device)
    sad = torch.full((30,), 7, dtype=torch.int32, device=ctx.device)
    sample = lambda graph, s, n, f, d: L.vgl_hip_sample_neighbors(ctx.h, graph.h, p(s), n, f, d, 0, p(srp), p(sad), None, None)
    assert sample(g, bad, 3, 10, 0) != 0 and b"seed" in L.vgl_hip_last_error()
    assert sample(g, neg, 3, 10, 0) != 0
    assert sample(g, seeds, 3, 0, 0) != 0 and b"fanout" in L.vgl_hip_last_error()
    assert sample(g, seeds, -1, 10, 0) != 0
    assert sample(g, seeds, 3, 10, 2) != 0
    assert sample(out_only, seeds, 3, 10, 1) != 0 and b"incoming" in L.vgl_hip_last_error()
    assert sample(shard, seeds, 3, 10, 0) != 0
    assert L.vgl_hip_sample_neighbors(ctx.h, g.h, p(seeds), 3, 10, 0, 0, None, p(sad), None, None) != 0
    ctx.sync()
    assert int((srp != 7).sum()) == 0 and int((sad != 7).sum()) == 0
    assert sample(g, seeds, 0, 10, 0) == 0 and srp.tolist() == [0, 7, 7, 7]      # no seeds: a success, rowptr[0] alone
    for call in (lambda: A.k_hop(g, [V], 1), lambda: A.sample_neighbors(g, [-1], 1), lambda: A.induced_subgraph(g, [V]),
                 lambda: A.edge_subgraph(g, torch.ones(g.E + 1)), lambda: A.induced_subgraph(g, torch.ones(V + 1, dtype=torch.bool)),
                 lambda: A.induced_subgraph(out_only, [0], with_incoming=True), lambda: A.k_hop(out_only, [0], 1, symmetric=True)):
        with pytest.raises(A._l.VglHipError):
            call()


# ---- 7. the scans: new_id from the vertex mask, rowptr from the row counts, the sampling rowptr, at the sizes around a scan's tile bounds ----
@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 2047, 2048, 2049, 70001])
def test_scans_across_sizes(V, ctx):
    A = api()
    L = ctx.L
    p = lambda t: C.c_void_p(t.data_ptr())
    v = np.arange(V, dtype=np.int64)
    chord = v[v % 5 == 0]
    src, dst = np.concatenate([v, chord]), np.concatenate([(v + 1) % V, (chord * 7 + 3) % V])      # a ring with a few chords
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    rowptr, adj, in_rowptr, in_adj = host(g)
    last = np.zeros(V, dtype=np.uint8)
    last[V - 1] = 1
    masks = {"all": np.ones(V, dtype=np.uint8), "none": np.zeros(V, dtype=np.uint8), "every third": (v % 3 == 0).astype(np.uint8), "the last": last}
    for name, keep in masks.items():
        what = "V = %d, keep %s" % (V, name)
        want_new = np.where(keep != 0, np.cumsum(keep) - keep, -1).astype(np.int32)
        want_old = np.nonzero(keep)[0].astype(np.int32)
        assert np.array_equal(want_new, R.vertex_maps(V, keep)[0])
        plan = C.c_void_p()
        A._l.check(L.vgl_hip_subgraph_plan_create(ctx.h, g.h, p(dev(ctx, keep, np.uint8)), None, C.byref(plan)))
        try:
            vk, eo, ei = C.c_int32(-1), C.c_int64(-1), C.c_int64(-1)
            A._l.check(L.vgl_hip_subgraph_plan_info(plan, C.byref(vk), C.byref(eo), C.byref(ei), None))
            assert vk.value == len(want_old), what
            new_id = torch.full((V,), 7, dtype=torch.int32, device=ctx.device)
            old_id = torch.full((max(vk.value, 1),), 7, dtype=torch.int32, device=ctx.device)
            A._l.check(L.vgl_hip_subgraph_plan_vertex_maps(ctx.h, plan, p(new_id), p(old_id)))
            assert np.array_equal(new_id.cpu().numpy(), want_new), what
            assert np.array_equal(old_id.cpu().numpy()[:vk.value], want_old), what
            for d, (rp_, ad_, kept) in enumerate(((rowptr, adj, eo.value), (in_rowptr, in_adj, ei.value))):
                row = R.rows_of(rp_)
                counts = np.bincount(want_new[row[(want_new[row] >= 0) & (want_new[ad_] >= 0)]], minlength=len(want_old))
                want_rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
                assert kept == want_rp[-1], (what, d)
                if vk.value == 0:
                    continue                                          # (a fill of V' = 0 writes nothing: test_refusals_write_nothing)
                assert np.array_equal(want_rp, R.filter_rows(rp_, ad_, keep)[0]), (what, d)
                rp = torch.full((vk.value + 1,), 7, dtype=torch.int64, device=ctx.device)
                ad = torch.full((max(kept, 1),), 7, dtype=torch.int32, device=ctx.device)
                A._l.check(L.vgl_hip_subgraph_plan_fill(ctx.h, plan, d, p(rp), p(ad), None))
                assert np.array_equal(rp.cpu().numpy(), want_rp), (what, d)
        finally:
            L.vgl_hip_subgraph_plan_destroy(ctx.h, plan)
    # V seeds, fanout 2: the sampling rowptr is the scan of min(degree, 2)
    seeds = ((v * 3 + 1) % V).astype(np.int32)
    for direction, rp_ in (("out", rowptr), ("in", in_rowptr)):
        if V <= 2049:
            rp = check_sample(g, seeds.tolist(), 2, 11, direction, what="V = %d" % V)[0]
        else:
            rp = A.sample_neighbors(g, seeds, 2, seed=11, direction=direction, raw=True)[0]
        deg = rp_[seeds.astype(np.int64) + 1] - rp_[seeds]
        assert np.array_equal(rp.cpu().numpy(), np.concatenate([[0], np.cumsum(np.minimum(deg, 2))])), (V, direction)


# ---- 8. the app ----
@pytest.mark.parametrize("mode", ["mask", "kcore", "hops", "sample"])
def test_subgraph_app(mode, tmp_path, ctx):
    dump = str(tmp_path / "subgraph.bin")
    extra = {"mask": ["-mask", "50"], "kcore": ["-kcore", "8"], "hops": ["-hops", "2", "-seeds", "4"], "sample": ["-sample", "10", "-seeds", "2000"]}[mode]
    cmd = [os.path.join(ROOT, "apps", "bin", "subgraph_hip"), "-gen", "-s", "10", "-e", "16", "-fused", "-check", "-dump", dump] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "error count: 0" in out.stdout and "error count" not in out.stdout.replace("error count: 0", ""), out.stdout
    assert os.path.getsize(dump) > 0 and os.path.getsize(dump) % 8 == 0
