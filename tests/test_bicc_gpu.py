"""Biconnectivity on the GPU (vgl_hip_bicc_run, api.biconnected_components / bridges / articulation_points / two_edge_connected_components,
apps/bin/bicc_hip) against the sequential restatement of the contract (tests/bicc_reference.py: a depth-first search, not the library's method),
closed forms and counts known by construction.  Every output is an integer and unique: everything is exact equality."""
import os
import subprocess

import numpy as np
import pytest
import torch

import bicc_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_SLOTS = ("bicc_flatten", "bicc_block", "bicc_art_short", "bicc_art_wave", "bicc_art_wg")
SLOTS = ("bicc_classify", "bicc_roots", "bicc_seed", "bicc_bfs_short", "bicc_bfs_wave", "bicc_bfs_wg", "bicc_publish", "bicc_size", "bicc_pre",
         "bicc_local_short", "bicc_local_wave", "bicc_local_wg", "bicc_lowhigh", "bicc_reset", "bicc_edge", "bicc_twoecc") + BLOCK_SLOTS
TENSORS = ("edges", "bridge", "edge_component", "articulation", "two_edge_component")
_REFS = {}


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def coo(ctx, src, dst):
    return (torch.tensor(np.asarray(src, dtype=np.int32), device=ctx.device), torch.tensor(np.asarray(dst, dtype=np.int32), device=ctx.device))


def reference(key, make):
    """(V, src, dst, the one reference result) under `key`: computed once, shared, left unchanged"""
    if key not in _REFS:
        V, src, dst = make()
        src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        _REFS[key] = (V, src, dst, R.biconnected(V, src, dst))
    return _REFS[key]


def block_graph(seed, blocks, hub_share):
    V, src, dst, ref = reference(("block", seed), lambda: R.block_graph(seed, blocks, hub_share)[:3])
    return V, src, dst, ref, R.block_graph(seed, blocks, hub_share)[3]


def generated(ctx, kind, scale, ef, seed):
    def make():
        src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
        return 1 << scale, src.cpu().numpy(), dst.cpu().numpy()
    return reference((kind, scale, ef, seed), make)


def own_depth(g, V, src, dst, ref):
    """depth counts the levels from the smallest vertex of every component IN THE GRAPH'S OWN NUMBERING: under a renumbering the reference is asked
    again on the relabelled entries"""
    if g.fwd is None:
        return ref["depth"]
    fwd = g.fwd.cpu().numpy().astype(np.int64)
    return R.biconnected(V, fwd[src], fwd[dst])["depth"]


def assert_equals_reference(g, V, src, dst, ref, what):
    """the five outputs and the integer statistics of one full run against the one reference result"""
    count, st = api().biconnected_components(g)
    print(what, {k: v for k, v in st.items() if not torch.is_tensor(v)})
    E = ref["edge_u"].size
    assert st["edges"].dtype == st["edge_component"].dtype == st["two_edge_component"].dtype == torch.int32, what
    assert st["bridge"].dtype == st["articulation"].dtype == torch.bool, what
    assert tuple(st["edges"].shape) == (E, 2) and np.array_equal(st["edges"].cpu().numpy(), np.stack([ref["edge_u"], ref["edge_v"]], axis=1)), what
    assert np.array_equal(st["bridge"].cpu().numpy(), ref["bridge"]), what
    assert np.array_equal(st["edge_component"].cpu().numpy(), ref["edge_component"]), what
    assert np.array_equal(st["articulation"].cpu().numpy(), ref["articulation"]), what
    assert np.array_equal(st["two_edge_component"].cpu().numpy(), ref["two_edge_component"]), what
    depth = own_depth(g, V, src, dst, ref)
    for k in R.INT_STATS:
        assert st[k] == (depth if k == "depth" else ref[k]), (what, k, st[k], ref[k])
    assert count == ref["biconnected_components"], what
    assert st["algorithmic_bytes"] == R.algorithmic_bytes(V, E, depth), what
    return st


def launches(ctx):
    return {n: ctx.timing_get(n)[0] for n in SLOTS}


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
@pytest.mark.parametrize("renumber", [None, "total"])
def test_hand_cases(name, renumber, ctx):
    V, stored, want = R.HAND_CASES[name]
    src, dst = np.asarray([a for a, _ in stored], dtype=np.int64), np.asarray([b for _, b in stored], dtype=np.int64)
    ref = R.biconnected(V, src, dst)
    for got, exp in zip((ref[k] for k in ("bridge", "edge_component", "articulation", "two_edge_component")), R.expected_arrays(V, stored, want)):
        assert np.array_equal(got, exp), name
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber=renumber)
    assert_equals_reference(g, V, src, dst, ref, name)
    g.close()


def _path(n):
    return n, np.arange(n - 1), np.arange(1, n)


def _cycle(n):
    return n, np.arange(n), (np.arange(n) + 1) % n


def _ladder(n):
    a = np.arange(n - 1)
    return 2 * n, np.concatenate([a, a + n, np.arange(n)]), np.concatenate([a + 1, a + n + 1, np.arange(n) + n])


def _necklace(n):
    """n triangles (3 i, 3 i + 1, 3 i + 2), triangle i joined to triangle i + 1 by the bridge (3 i + 2, 3 i + 3)"""
    t = 3 * np.arange(n)
    b = 3 * np.arange(n - 1)
    return 3 * n, np.concatenate([t, t + 1, t + 2, b + 2]), np.concatenate([t + 1, t + 2, t, b + 3])


def _star(n):
    return n + 1, np.zeros(n, dtype=np.int64), np.arange(1, n + 1)


def _binary_tree(depth):
    n = (1 << (depth + 1)) - 1
    c = np.arange(1, n)
    return n, (c - 1) // 2, c


# name -> (graph, expected depth, bridges, cut vertices, blocks, 2-edge-connected components, edges of the largest block)
CLOSED_FORMS = {
    "path_3000": (lambda: _path(3000), 3000, 2999, 2998, 2999, 3000, 1),
    "cycle_3000": (lambda: _cycle(3000), 1501, 0, 0, 1, 1, 3000),
    "ladder_2x1500": (lambda: _ladder(1500), 1501, 0, 0, 1, 1, 4498),
    "necklace_500": (lambda: _necklace(500), 1000, 499, 998, 999, 500, 3),
    "star_5000": (lambda: _star(5000), 2, 5000, 1, 5000, 5001, 1),
    "binary_tree_12": (lambda: _binary_tree(12), 13, 8190, 4095, 8190, 8191, 1),
}


@pytest.mark.parametrize("name", sorted(CLOSED_FORMS))
def test_closed_forms_where_the_level_loops_can_go_wrong(name, ctx):
    make, depth, bridges, cuts, blocks, two, largest = CLOSED_FORMS[name]
    V, src, dst, ref = reference(("closed", name), make)
    assert (ref["depth"], ref["bridges"], ref["articulation_points"], ref["biconnected_components"], ref["two_edge_components"], ref["largest_component_edges"]) == \
        (depth, bridges, cuts, blocks, two, largest), name
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst), with_incoming=False)
    ctx.timing(True)
    st = assert_equals_reference(g, V, src, dst, ref, name)
    n = launches(ctx)
    ctx.timing(False)
    print(name, n)
    assert st["components"] == 1
    # every turn of the host loop advances a level: one expansion per level (the last finds nothing), one launch per level of the passes up and down
    assert n["bicc_bfs_short"] + n["bicc_bfs_wave"] + n["bicc_bfs_wg"] == depth, n
    assert n["bicc_pre"] == depth and n["bicc_size"] == n["bicc_lowhigh"] == depth - 1, n
    assert n["bicc_publish"] == depth + 3, n                                     # the classes, the seed, one per level, the totals
    if name == "star_5000":                                                      # the hub is a workgroup row at the default thresholds
        assert n["bicc_bfs_wg"] == n["bicc_local_wg"] == n["bicc_art_wg"] == 1 and n["bicc_bfs_wave"] == 0, n
    g.close()


BLOCK_GRAPHS = [(1, 300, 0.0), (2, 300, 0.3), (3, 1000, 0.05)]


@pytest.mark.parametrize("seed,blocks,hub_share", BLOCK_GRAPHS)
def test_block_graphs(seed, blocks, hub_share, ctx):
    """the directed graph, the symmetrised graph (no incoming CSR) and the renumbered graph: one reference result, and the counts of the construction"""
    A = api()
    V, src, dst, ref, expect = block_graph(seed, blocks, hub_share)
    assert {k: ref[k] for k in expect} == expect
    s, d = coo(ctx, src, dst)
    g = A.Graph.from_coo(ctx, V, s, d)
    st = assert_equals_reference(g, V, src, dst, ref, "directed")
    assert {k: st[k] for k in expect} == expect
    g.close()
    y = A.Graph.from_coo(ctx, V, torch.cat([s, d]), torch.cat([d, s]), with_incoming=False)
    assert_equals_reference(y, V, src, dst, ref, "symmetrised")
    y.close()
    r = A.Graph.from_coo(ctx, V, s, d, renumber="total")
    st = assert_equals_reference(r, V, src, dst, ref, "renumbered")
    assert {k: st[k] for k in expect} == expect
    _, raw = A.biconnected_components(r, raw=True)                               # the graph's own numbering and edge order
    bwd = r.bwd.cpu().numpy().astype(np.int64)
    fwd = r.fwd.cpu().numpy().astype(np.int64)
    e = raw["edges"].cpu().numpy().astype(np.int64)
    assert bool((e[:, 0] < e[:, 1]).all()) and bool((np.diff(e[:, 0] * V + e[:, 1]) > 0).all())
    a, b = bwd[e[:, 0]], bwd[e[:, 1]]
    key = np.minimum(a, b) * V + np.maximum(a, b)
    ref_key = ref["edge_u"].astype(np.int64) * V + ref["edge_v"]
    at = np.searchsorted(ref_key, key)                                           # every raw edge is one of the reference's, in ORIGINAL ids
    assert np.unique(key).size == ref_key.size and np.array_equal(ref_key[at], key)
    assert np.array_equal(raw["bridge"].cpu().numpy(), ref["bridge"][at])
    lab = raw["edge_component"].cpu().numpy()
    assert np.array_equal(lab[lab], lab) and bool((lab <= np.arange(lab.size)).all())      # the smallest edge id of the block, in the raw order
    want = np.full(at.size, at.size, dtype=np.int64)                             # the reference's blocks, named by the smallest RAW id
    np.minimum.at(want, ref["edge_component"][at], np.arange(at.size))
    assert np.array_equal(lab, want[ref["edge_component"][at]])
    assert np.array_equal(raw["articulation"].cpu().numpy(), ref["articulation"][bwd])
    two = raw["two_edge_component"].cpu().numpy().astype(np.int64)
    smallest = np.full(V, V, dtype=np.int64)                                     # the reference's components, named by the smallest OWN id
    np.minimum.at(smallest, ref["two_edge_component"], fwd)
    assert np.array_equal(two, smallest[ref["two_edge_component"][bwd]])
    r.close()


GENERATED = [("uniform", 12, 1, 1, True), ("rmat", 12, 2, 1, True), ("rmat", 10, 16, 1, False)]


@pytest.mark.parametrize("kind,scale,ef,seed,sparse", GENERATED)
def test_generated_graphs(kind, scale, ef, seed, sparse, ctx):
    A = api()
    V, src, dst, ref = generated(ctx, kind, scale, ef, seed)
    if sparse:                                                                   # bridges and cut vertices abound beside one giant block
        assert ref["bridges"] >= 100 and ref["articulation_points"] >= 100 and ref["largest_component_edges"] >= 1000, {k: ref[k] for k in R.INT_STATS}
    s, d = coo(ctx, src, dst)
    g = A.Graph.from_coo(ctx, V, s, d)
    assert_equals_reference(g, V, src, dst, ref, "directed")
    g.close()
    r = A.Graph.from_coo(ctx, V, s, d, renumber="total")
    assert_equals_reference(r, V, src, dst, ref, "renumbered")
    r.close()


SHRUNK = {"VGL_BICC_SHORT": "2", "VGL_BICC_WAVE": "8"}


def test_every_class_with_shrunk_thresholds(ctx, monkeypatch):
    A = api()
    V, src, dst, ref, _ = block_graph(2, 300, 0.3)
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    ctx.timing(True)
    st0 = assert_equals_reference(g, V, src, dst, ref, "default thresholds")
    n0 = launches(ctx)
    assert st0["prepared_now"] == 1
    for k, v in SHRUNK.items():
        monkeypatch.setenv(k, v)
    ctx.timing(True)
    st1 = assert_equals_reference(g, V, src, dst, ref, "shrunk thresholds, cached prepare")
    n1 = launches(ctx)
    ctx.timing(False)
    print("launches under the default / shrunk thresholds", n0, n1)
    assert st1["prepared_now"] == 0
    assert all(n1[k] > 0 for k in SLOTS), n1
    assert n0["bicc_local_wg"] == 0 and n0["bicc_local_short"] == 1, n0
    assert all(torch.equal(st0[k], st1[k]) for k in TENSORS)
    assert all(st0[k] == st1[k] for k in R.INT_STATS + ("algorithmic_bytes",)), (st0, st1)
    g.close()


def test_two_runs_agree_and_prepare_is_cached(ctx):
    A = api()
    V, src, dst, ref = generated(ctx, "rmat", 12, 2, 1)
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    _, s0 = A.biconnected_components(g)
    _, s1 = A.biconnected_components(g)
    assert s0["prepared_now"] == 1 and s1["prepared_now"] == 0
    assert all(torch.equal(s0[k], s1[k]) for k in TENSORS)
    assert all(s0[k] == s1[k] for k in R.INT_STATS + ("algorithmic_bytes",)), (s0, s1)
    g.close()
    p = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    assert p.prepare_bicc() == ref["edge_u"].size
    _, s2 = A.biconnected_components(p)
    assert s2["prepared_now"] == 0 and all(torch.equal(s0[k], s2[k]) for k in TENSORS)
    p.close()


# RMAT-20x16, seed 1: what apps/bin/bicc_hip -check confirmed against its sequential host Hopcroft-Tarjan on this graph (the Python restatement would
# take minutes here).  The size is the one at which a second run in one process once refused with an internal error.
RMAT20 = {"undirected_edges": 15937349, "components": 377754, "bridges": 140845, "articulation_points": 57656, "biconnected_components": 140846,
          "two_edge_components": 518599, "largest_component_edges": 15796504, "depth": 7}


def test_back_to_back_runs_at_scale_20(ctx):
    """six runs on one handle, then the app (three runs of its own in one process) twice: the same outputs and statistics every time"""
    A = api()
    V = 1 << 20
    src, dst = ctx.gen_rmat(20, 16, 1)
    g = A.Graph.from_coo(ctx, V, src, dst, with_incoming=False)
    del src, dst
    _, first = A.biconnected_components(g, raw=True)
    assert {k: first[k] for k in RMAT20} == RMAT20
    assert first["algorithmic_bytes"] == R.algorithmic_bytes(V, RMAT20["undirected_edges"], RMAT20["depth"])
    assert int(first["bridge"].sum()) == RMAT20["bridges"] and int(first["articulation"].sum()) == RMAT20["articulation_points"]
    assert int(torch.unique(first["edge_component"]).numel()) == RMAT20["biconnected_components"]
    assert int(torch.unique(first["two_edge_component"]).numel()) == RMAT20["two_edge_components"]
    for run in range(5):
        _, again = A.biconnected_components(g, raw=True)
        assert all(torch.equal(first[k], again[k]) for k in TENSORS), run
        assert all(first[k] == again[k] for k in R.INT_STATS + ("algorithmic_bytes",)), (run, again)
    g.close()
    for run in range(2):
        out = subprocess.run([os.path.join(ROOT, "apps", "bin", "bicc_hip"), "-gen", "-s", "20", "-e", "16", "-fused"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.count("BICC: 140846 blocks") == 2, out.stdout[-2000:] + out.stderr[-500:]


def test_partial_requests_skip_the_block_pass(ctx):
    A = api()
    V, src, dst, ref, _ = block_graph(1, 300, 0.0)
    E = ref["edge_u"].size
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber="total")
    _, full = A.biconnected_components(g)
    depth = full["depth"]
    ctx.timing(True)
    st = A._bicc(g, False, edges=True, bridge=True)
    n = launches(ctx)
    ctx.timing(False)
    assert st["biconnected_components"] == st["articulation_points"] == st["largest_component_edges"] == -1
    assert all(n[k] == 0 for k in BLOCK_SLOTS) and n["bicc_twoecc"] == 0 and n["bicc_reset"] == 0 and n["bicc_edge"] == 1, n
    assert st["bridges"] == ref["bridges"] and st["two_edge_components"] == ref["two_edge_components"] and st["components"] == ref["components"]
    assert st["algorithmic_bytes"] == R.algorithmic_bytes(V, E, depth, edges=True, bridge=True, blocks=False, two_edge=False)
    assert torch.equal(st["bridge"], full["bridge"]) and torch.equal(st["edges"], full["edges"])
    got = A.bridges(g)
    assert got.dtype == torch.int32 and torch.equal(got, full["edges"][full["bridge"]])
    assert np.array_equal(got.cpu().numpy(), np.stack([ref["edge_u"], ref["edge_v"]], axis=1)[ref["bridge"]])
    cuts = A.articulation_points(g)
    assert np.array_equal(cuts.cpu().numpy(), np.flatnonzero(ref["articulation"]))
    ctx.timing(True)
    two = A.two_edge_connected_components(g)
    n = launches(ctx)
    ctx.timing(False)
    assert all(n[k] == 0 for k in BLOCK_SLOTS) and n["bicc_twoecc"] == n["bicc_reset"] == 1, n
    assert two.dtype == torch.int32 and np.array_equal(two.cpu().numpy(), ref["two_edge_component"])
    g.close()


@pytest.mark.parametrize("first", ["ktruss", "bicc"])
def test_bicc_and_ktruss_share_the_edge_numbering(first, ctx):
    A = api()
    V, src, dst, ref = generated(ctx, "rmat", 10, 16, 1)
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    ctx.timing(True)
    if first == "ktruss":
        _, kt = A.truss_numbers(g)
        bi = assert_equals_reference(g, V, src, dst, ref, "after ktruss")
        assert kt["prepared_now"] == 1 and bi["prepared_now"] == 0
    else:
        bi = assert_equals_reference(g, V, src, dst, ref, "before ktruss")
        _, kt = A.truss_numbers(g)
        assert bi["prepared_now"] == 1 and kt["prepared_now"] == 0
    built = ctx.timing_get("kcore_csr")[0]
    ctx.timing(False)
    assert built == 1, built                                                     # the symmetric CSR was built once for the two of them
    assert torch.equal(kt["edges"], bi["edges"]) and kt["undirected_edges"] == bi["undirected_edges"]
    g.close()


def test_cross_checks_with_cc_and_msf(ctx):
    A = api()
    V, src, dst, ref = generated(ctx, "uniform", 12, 1, 1)
    s, d = coo(ctx, src, dst)
    y = A.Graph.from_coo(ctx, V, torch.cat([s, d]), torch.cat([d, s]), with_incoming=False)
    _, bi = A.biconnected_components(y)
    labels = A.connected_components(y)[0]
    assert bi["components"] == int(torch.unique(labels).numel())
    for seed in (1, 2):                                                          # a bridge is in every spanning forest, whatever the weights
        w = ctx.gen_weights(y.E, seed)
        _, ms = A.minimum_spanning_forest(y, w)
        assert torch.equal(ms["all_edges"], bi["edges"])
        assert bi["bridges"] <= ms["forest_edges"] and bool(ms["in_forest"][bi["bridge"]].all())
    y.close()


def test_refusals_write_nothing(ctx):
    A = api()
    V, src, dst, ref, _ = block_graph(1, 300, 0.0)
    E = ref["edge_u"].size
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    sh = g.shard(0, V // 2)
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        A.biconnected_components(sh)
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        sh.prepare_bicc()
    i32 = [torch.full((max(E, V),), 0x5A5A5A5A, dtype=torch.int32, device=ctx.device) for _ in range(4)]
    u8 = [torch.full((max(E, V),), 0x5A, dtype=torch.uint8, device=ctx.device) for _ in range(2)]
    eu, ev, lab, two = [A._ptr(t) for t in i32]
    br, art = [A._ptr(t) for t in u8]
    with pytest.raises(A._l.VglHipError, match="all outputs are NULL"):
        A._l.check(ctx.L.vgl_hip_bicc_run(ctx.h, g.h, None, None, None, None, None, None, None))
    with pytest.raises(A._l.VglHipError, match="d_edge_u and d_edge_v"):
        A._l.check(ctx.L.vgl_hip_bicc_run(ctx.h, g.h, eu, None, br, lab, art, two, None))
    with pytest.raises(A._l.VglHipError, match="d_edge_u and d_edge_v"):
        A._l.check(ctx.L.vgl_hip_bicc_run(ctx.h, g.h, None, ev, br, lab, art, two, None))
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        A._l.check(ctx.L.vgl_hip_bicc_run(ctx.h, sh.h, eu, ev, br, lab, art, two, None))
    ctx.sync()
    assert all(bool((t == 0x5A5A5A5A).all()) for t in i32) and all(bool((t == 0x5A).all()) for t in u8)
    A._l.check(ctx.L.vgl_hip_bicc_run(ctx.h, g.h, None, None, br, None, None, None, None))      # one output is enough
    assert np.array_equal(u8[0][:E].cpu().numpy().astype(bool), ref["bridge"]) and bool((u8[0][E:] == 0x5A).all())
    for h in (sh, g):
        h.close()


def test_bicc_app(tmp_path, ctx):
    dump = str(tmp_path / "bicc.bin")
    cmd = [os.path.join(ROOT, "apps", "bin", "bicc_hip"), "-gen", "-s", "12", "-e", "2", "-fused", "-check", "-format", "vcsr", "-dump", dump]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "error count: 0" in out.stdout and "error count" not in out.stdout.replace("error count: 0", ""), out.stdout
    A = api()
    src, dst = ctx.gen_rmat(12, 2, 1)                                            # what -gen generates: the app's default seed, the same generator
    g = A.Graph.from_coo(ctx, 1 << 12, src, dst, renumber="total")
    _, st = A.biconnected_components(g)
    want = torch.cat([st["edges"], st["edge_component"][:, None], st["bridge"].to(torch.int32)[:, None]], dim=1).cpu().numpy()
    assert np.array_equal(np.fromfile(dump, np.int32).reshape(-1, 4), want)
    g.close()
