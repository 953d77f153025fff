"""Multi-source BFS on the GPU (vgl_hip_msbfs_run, api.multi_source_bfs and the three centralities on top of it, apps/bin/closeness_hip) against the
numpy / scipy restatement of the contract (tests/msbfs_reference.py) and closed forms.  Everything is compared for equality, harmonic bit for bit; only
the comparison with networkx, which adds in another order, has a bound: V * 2^-52 relative."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import msbfs_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("reached", "dist_sum", "ecc", "harmonic")
PUSH_STATS = ("edges_push", "levels_total", "reached_total")
SLOTS = ["msbfs_%s_%s" % (w, k) for w in ("push", "pull") for k in ("short", "wave", "wg")]


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def coo(ctx, src, dst):
    return (torch.tensor(np.asarray(src, dtype=np.int32), device=ctx.device), torch.tensor(np.asarray(dst, dtype=np.int32), device=ctx.device))


def same_bits(got, want):
    """equality of two arrays; float64 compared as the 64-bit patterns"""
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype == np.float64:
        return got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64))
    return got.dtype == want.dtype and np.array_equal(got, want)


def assert_equals_reference(g, V, src, dst, sources, what, direction="out", symmetric=False, levels=True, ref=None):
    """the four per-source outputs, the levels and the schedule-independent stats of one API call against the restatement on the ORIGINAL ids"""
    A = api()
    ref = R.multi_source_bfs(V, src, dst, range(V) if sources is None else sources, direction, want_levels=levels) if ref is None else ref
    got, st = A.multi_source_bfs(g, sources, direction=direction, symmetric=symmetric, want_levels=levels)
    print(what, st)
    for k in KEYS:
        assert same_bits(got[k].cpu().numpy(), ref[k]), (what, k)
    if levels:
        assert got["levels"].dtype == torch.int32 and np.array_equal(got["levels"].cpu().numpy(), ref["levels"]), what
    n = V if sources is None else len(sources)
    assert st["sources"] == n and st["batches"] == ref["batches"] == -(-n // 64) and st["max_depth"] == ref["max_depth"]
    assert st["levels_total"] == ref["levels_total"] and st["reached_total"] == ref["reached_total"]
    assert st["levels_push"] + st["levels_pull"] == st["levels_total"]
    return got, st, ref


def pick_sources(V, src, dst, count, seed):
    """vertex 0 (a hub), a vertex without outgoing entries, one without incoming entries (where they exist), the rest seeded"""
    outdeg, indeg = np.bincount(src, minlength=V), np.bincount(dst, minlength=V)
    chosen = [0]
    for deg in (outdeg, indeg):
        none = np.flatnonzero(deg == 0)
        if none.size and int(none[0]) not in chosen:
            chosen.append(int(none[0]))
    for v in np.random.default_rng(seed).permutation(V).tolist():
        if len(chosen) >= count:
            break
        if v not in chosen:
            chosen.append(v)
    return chosen


@pytest.fixture(scope="module")
def rmat10(ctx):
    V = 1 << 10
    src, dst = ctx.gen_rmat(10, 8, 2)
    s_np, d_np = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
    g = api().Graph.from_coo(ctx, V, src, dst)
    everything = R.multi_source_bfs(V, s_np, d_np, range(V))               # computed once, shared, left unchanged
    yield V, s_np, d_np, g, everything
    g.close()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130, 1 << 10])
def test_batch_edges(count, rmat10):
    """a single source, one short of a word, a full word, one over, two words and a partial one, every vertex: the partial last batch leaks nothing"""
    V, s_np, d_np, g, everything = rmat10
    if count == V:
        assert_equals_reference(g, V, s_np, d_np, None, "every vertex", ref=everything)
        return
    sources = pick_sources(V, s_np, d_np, count, count)
    # the restatement's answers do not depend on the batch a source is in: take them from the shared run, the batch-dependent stats from a run of its own
    ref = R.multi_source_bfs(V, s_np, d_np, sources)
    for k in KEYS + ("levels",):
        assert np.array_equal(ref[k], everything[k][sources]), k
    assert_equals_reference(g, V, s_np, d_np, sources, "%d sources" % count, ref=ref)


def test_every_bit_has_its_own_answer(ctx):
    """source j of the batch is vertex j of a directed 64-path inside a graph of 100 vertices (no multiple of 64): bit b reaches 64 - b vertices, bit 63
    its source alone -- a 32-bit shift would fold the upper half onto the lower.  The second, partial batch repeats the sources in reverse."""
    V = 100
    src, dst = np.arange(63), np.arange(1, 64)
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    sources = list(range(64)) + list(range(63, 30, -1))
    got, _, _ = assert_equals_reference(g, V, src, dst, sources, "64-path")
    want = np.array([64 - s for s in sources])
    assert np.array_equal(got["reached"].cpu().numpy(), want) and np.array_equal(got["ecc"].cpu().numpy(), want - 1)
    assert np.array_equal(got["dist_sum"].cpu().numpy(), (want - 1) * want // 2)
    back, _, _ = assert_equals_reference(g, V, src, dst, sources, "64-path, incoming", direction="in")
    assert np.array_equal(back["reached"].cpu().numpy(), np.array([s + 1 for s in sources]))
    g.close()


def test_duplicates_sinks_loops_and_multi_edges(ctx):
    """duplicate sources inside one batch and across two, a source without outgoing entries, an isolated vertex, self-loops, multi-edges"""
    rng = np.random.default_rng(21)
    V = 131
    src, dst = rng.integers(0, 120, 500), rng.integers(0, 120, 500)       # 120 .. 130 get nothing from here
    dup = rng.integers(0, 500, 150)
    loops = np.array([0, 5, 5, 121, 77])
    src = np.concatenate([src, src[dup], loops, [3, 3, 3]])
    dst = np.concatenate([dst, dst[dup], loops, [125, 125, 126]])         # 125 and 126: reached, no outgoing entries; 121: only its loop; 130: isolated
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    sources = [7, 7, 125, 130, 121, 3] + list(range(60)) + [7, 3, 130, 7] + list(range(60, 120))
    for direction in ("out", "in"):
        got, _, _ = assert_equals_reference(g, V, src, dst, sources, "odd ends, " + direction, direction=direction)
        for k in KEYS:
            r = got[k].cpu().numpy()
            assert r[0] == r[1] == r[66] == r[69], k                       # the same source four times: four traversals, one answer
    assert int(got["reached"][3]) == 1 and int(got["ecc"][3]) == 0 and float(got["harmonic"][3]) == 0.0
    g.close()


def test_one_vertex_and_no_edges(ctx):
    A = api()
    g = A.Graph.from_coo(ctx, 1, *coo(ctx, [0], [0]))
    got, st, _ = assert_equals_reference(g, 1, np.array([0]), np.array([0]), [0, 0], "V = 1")
    assert got["reached"].tolist() == [1, 1] and st["levels_total"] == 1
    g.close()
    empty = np.zeros(0, dtype=np.int64)
    g = A.Graph.from_coo(ctx, 70, *coo(ctx, empty, empty))
    got, st, _ = assert_equals_reference(g, 70, empty, empty, None, "E = 0")
    assert bool((got["reached"] == 1).all()) and st["levels_total"] == 2 and st["edges_push"] == 0
    g.close()


GRAPHS = [("rmat", 12, 16, 2, 130), ("rmat", 14, 16, 3, 65), ("uniform", 12, 16, 5, 65)]


@pytest.mark.parametrize("kind,scale,ef,seed,count", GRAPHS)
def test_generated_graphs(kind, scale, ef, seed, count, ctx):
    """directed along outgoing and along incoming entries, renumbered, and symmetrised without an incoming CSR; levels against api.bfs"""
    A = api()
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    s_np, d_np = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
    sources = pick_sources(V, s_np, d_np, count, seed)
    g = A.Graph.from_coo(ctx, V, src, dst)
    out, _, ref_out = assert_equals_reference(g, V, s_np, d_np, sources, "directed, out")
    inn, _, ref_in = assert_equals_reference(g, V, s_np, d_np, sources, "directed, in", direction="in")
    for j in range(0, len(sources), max(1, len(sources) // 8))[:8]:
        single, _ = A.bfs(g, sources[j])
        assert torch.equal(out["levels"][j], single), sources[j]
    g.close()
    r = A.Graph.from_coo(ctx, V, src, dst, renumber="total")
    for direction, first, ref in (("out", out, ref_out), ("in", inn, ref_in)):
        got, _, _ = assert_equals_reference(r, V, s_np, d_np, sources, "renumbered, " + direction, direction=direction, ref=ref)
        for k in KEYS + ("levels",):
            assert torch.equal(got[k], first[k]), k
    raw, _ = A.multi_source_bfs(r, [r.vertex_id(s) for s in sources], want_levels=True, raw=True)      # the graph's own numbering
    assert torch.equal(raw["reached"], out["reached"]) and torch.equal(raw["levels"], out["levels"][:, r.bwd.long()])
    r.close()
    both = (torch.cat([src, dst]), torch.cat([dst, src]))
    b_s, b_d = np.concatenate([s_np, d_np]), np.concatenate([d_np, s_np])
    s = A.Graph.from_coo(ctx, V, *both, with_incoming=False)
    sym_sources = pick_sources(V, b_s, b_d, count, seed)
    got, st, ref = assert_equals_reference(s, V, b_s, b_d, sym_sources, "symmetrised", symmetric=True)
    back, _, _ = assert_equals_reference(s, V, b_s, b_d, sym_sources, "symmetrised, in", direction="in", symmetric=True, ref=ref)
    assert st["levels_pull"] > 0                                           # the outgoing CSR serves the pull as well
    s.close()


def run_mode(monkeypatch, mode, g, sources, **kw):
    if mode is None:
        monkeypatch.delenv("VGL_MSBFS_MODE", raising=False)
    else:
        monkeypatch.setenv("VGL_MSBFS_MODE", mode)
    return api().multi_source_bfs(g, sources, want_levels=True, **kw)


def test_schedules_give_identical_outputs(ctx, monkeypatch):
    A = api()
    V = 1 << 14
    src, dst = ctx.gen_rmat(14, 16, 3)
    s_np, d_np = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
    sources = pick_sources(V, s_np, d_np, 65, 3)
    g = A.Graph.from_coo(ctx, V, src, dst)
    for direction in ("out", "in"):
        ref = R.multi_source_bfs(V, s_np, d_np, sources, direction)
        res = {m: run_mode(monkeypatch, m, g, sources, direction=direction) for m in ("push", "pull", "auto", None)}
        for m, (got, st) in res.items():
            print(direction, m, st)
            for k in KEYS + ("levels",):
                assert torch.equal(got[k], res["push"][0][k]), (direction, m, k)
                assert same_bits(got[k].cpu().numpy(), ref[k]), (direction, m, k)
        st = res["push"][1]
        assert st["levels_pull"] == 0 and st["edges_pull"] == 0
        for k in PUSH_STATS:
            assert st[k] == ref[k], (direction, k, st[k], ref[k])
        assert res["pull"][1]["levels_push"] == 0 and res["pull"][1]["edges_push"] == 0
        assert res["auto"][1] == res[None][1]
        assert res["auto"][1]["levels_push"] > 0 and res["auto"][1]["levels_pull"] > 0, res["auto"][1]
    monkeypatch.delenv("VGL_MSBFS_MODE", raising=False)
    no_in = A.Graph.from_coo(ctx, V, src, dst, with_incoming=False)
    got, st = A.multi_source_bfs(no_in, sources, want_levels=True)         # no reverse CSR: push only, the same answers
    assert st["levels_pull"] == 0 and st["levels_push"] == st["levels_total"]
    ref = R.multi_source_bfs(V, s_np, d_np, sources)
    for k in KEYS + ("levels",):
        assert same_bits(got[k].cpu().numpy(), ref[k]), k
    for k in PUSH_STATS:
        assert st[k] == ref[k], k
    monkeypatch.setenv("VGL_MSBFS_MODE", "pull")
    with pytest.raises(A._l.VglHipError, match="reverse CSR"):
        A.multi_source_bfs(no_in, sources)
    monkeypatch.setenv("VGL_MSBFS_MODE", "sideways")
    with pytest.raises(A._l.VglHipError, match="VGL_MSBFS_MODE"):
        A.multi_source_bfs(g, sources)
    for h in (g, no_in):
        h.close()


def launches(ctx):
    return {k: ctx.timing_get(k)[0] for k in SLOTS}


def test_every_row_class_with_shrunk_thresholds(ctx, monkeypatch):
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 11)
    s_np, d_np = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
    sources = pick_sources(V, s_np, d_np, 70, 11)
    g = A.Graph.from_coo(ctx, V, src, dst)
    first, st, ref = assert_equals_reference(g, V, s_np, d_np, sources, "default thresholds")
    assert st["prepared_now"] == 1
    g.close()
    for k, v in {"VGL_MSBFS_SHORT": "4", "VGL_MSBFS_WAVE": "16", "VGL_MSBFS_CHUNK": "16"}.items():
        monkeypatch.setenv(k, v)
    g = A.Graph.from_coo(ctx, V, src, dst)                                 # a new handle under the shrunk switches
    ctx.timing(True)
    for mode in ("push", "pull", "auto"):
        monkeypatch.setenv("VGL_MSBFS_MODE", mode)
        got, _, _ = assert_equals_reference(g, V, s_np, d_np, sources, "shrunk thresholds, " + mode, ref=ref)
        for k in KEYS + ("levels",):
            assert torch.equal(got[k], first[k]), (mode, k)
    n = launches(ctx)
    ctx.timing(False)
    print("launches", n)
    assert all(v > 0 for v in n.values()), n
    g.close()


def test_hub_star(ctx, monkeypatch):
    """centre 0 and 2^17 leaves, stored both ways: one row of 2^17 entries (the chunked class under the default switches) in push and in pull"""
    A = api()
    k = 1 << 17
    leaves = np.arange(1, k + 1)
    src, dst = np.concatenate([np.zeros(k, dtype=np.int64), leaves]), np.concatenate([leaves, np.zeros(k, dtype=np.int64)])
    g = A.Graph.from_coo(ctx, k + 1, *coo(ctx, src, dst))
    sources = [0, 1, 2, k]
    ref = R.multi_source_bfs(k + 1, src, dst, sources, want_levels=False)
    leaf_h = float(np.float64(1.0) / np.float64(1.0) + np.float64(k - 1) / np.float64(2.0))
    for mode in ("push", "pull"):
        monkeypatch.setenv("VGL_MSBFS_MODE", mode)
        ctx.timing(True)
        got, st = A.multi_source_bfs(g, sources)
        n = launches(ctx)
        ctx.timing(False)
        print(mode, st, n)
        assert n["msbfs_%s_wg" % mode] > 0, n
        assert got["reached"].tolist() == [k + 1] * 4 and got["dist_sum"].tolist() == [k] + [1 + 2 * (k - 1)] * 3
        assert got["ecc"].tolist() == [1, 2, 2, 2] and got["harmonic"].tolist() == [float(k)] + [leaf_h] * 3
        assert st["levels_total"] == 3 and st["reached_total"] == 4 * (k + 1)
        if mode == "push":                                                  # the centre and three leaves; the centre and all leaves; all leaves
            assert st["edges_push"] == (k + 3) + 2 * k + k == ref["edges_push"]
    g.close()


def test_deep_path_costs_its_entries_not_depth_times_v(ctx):
    """a directed path of 5000 vertices, sources [0, 2500, 4999, 0], the default schedule: one settle launch per level, over the new list and not over V.
    edges_push: vertex k carries sources 0 and 3 at level k and is counted once (4999 vertices with an entry); vertex 2500 + k carries source 1
    (2499 with an entry); the two frontier vertices never meet, so the sum is 7498 -- what the restatement gives.  (4999 would be the figure if source
    2500's own frontier walked nothing.)"""
    A = api()
    n = 5000
    src, dst = np.arange(n - 1), np.arange(1, n)
    g = A.Graph.from_coo(ctx, n, *coo(ctx, src, dst))
    sources = [0, 2500, 4999, 0]
    ref = R.multi_source_bfs(n, src, dst, sources, want_levels=False)
    ctx.timing(True)
    got, st, _ = assert_equals_reference(g, n, src, dst, sources, "path 5000", levels=False, ref=ref)
    settle, publish = ctx.timing_get("msbfs_settle")[0], ctx.timing_get("msbfs_publish")[0]
    ctx.timing(False)
    tri = lambda m: m * (m + 1) // 2
    assert got["reached"].tolist() == [n, n - 2500, 1, n] and got["dist_sum"].tolist() == [tri(n - 1), tri(n - 2501), 0, tri(n - 1)]
    assert got["ecc"].tolist() == [n - 1, n - 2501, 0, n - 1]
    assert st["levels_total"] == n and st["levels_pull"] == 0 and st["max_depth"] == n - 1
    assert st["edges_push"] == ref["edges_push"] == 4999 + 2499
    print("launches: settle", settle, "publish", publish)
    assert settle == st["levels_total"] and publish == st["levels_total"] + 1      # the seed's counters are read once more
    g.close()


def test_reproducible_and_prepared_once(ctx):
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 13)
    s_np, d_np = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
    g = A.Graph.from_coo(ctx, V, src, dst)
    g.prepare_msbfs("in")
    sources = pick_sources(V, s_np, d_np, 100, 13)
    one, st1 = A.multi_source_bfs(g, sources, direction="in", want_levels=True)
    two, st2 = A.multi_source_bfs(g, sources, direction="in", want_levels=True)
    assert st1["prepared_now"] == 0 and st2["prepared_now"] == 0 and st1 == st2
    for k in KEYS + ("levels",):
        assert torch.equal(one[k], two[k]), k
    assert torch.equal(one["harmonic"].view(torch.int64), two["harmonic"].view(torch.int64))
    g.close()


def raw_run(ctx, g, sources, direction, symmetric, bufs, count=None):
    A = api()
    n = len(sources)
    arr = (C.c_int32 * max(n, 1))(*sources)
    st = A._l.MsbfsStats()
    ptr = [None if b is None else C.c_void_p(b.data_ptr()) for b in bufs]
    A._l.check(ctx.L.vgl_hip_msbfs_run(ctx.h, g.h, arr, n if count is None else count, direction, int(symmetric), *ptr, C.byref(st)))
    ctx.sync()
    return st


def test_errors_leave_the_outputs_untouched(ctx):
    A = api()
    V = 1 << 10
    src, dst = ctx.gen_rmat(10, 8, 17)
    g = A.Graph.from_coo(ctx, V, src, dst)
    no_in = A.Graph.from_coo(ctx, V, src, dst, with_incoming=False)
    sh = g.shard(0, V // 2)
    bufs = [torch.full((2,), 7, dtype=torch.int64, device=ctx.device), torch.full((2,), 7, dtype=torch.int64, device=ctx.device),
            torch.full((2,), 7, dtype=torch.int32, device=ctx.device), torch.full((2,), 7.0, dtype=torch.float64, device=ctx.device),
            torch.full((2 * V,), 7, dtype=torch.int32, device=ctx.device)]
    untouched = lambda: all(bool((b == 7).all()) for b in bufs)
    cases = [(sh, [0], 0, False, "own all rows"), (sh, [0], 0, True, "own all rows"), (no_in, [0], 1, False, "incoming CSR"),
             (g, [0, V], 0, False, "out of range"), (g, [-1], 1, False, "out of range"), (g, [0], 2, False, "direction")]
    for handle, sources, direction, symmetric, message in cases:
        with pytest.raises(A._l.VglHipError, match=message):
            raw_run(ctx, handle, sources, direction, symmetric, bufs)
        assert untouched(), message
    with pytest.raises(A._l.VglHipError, match="count"):
        raw_run(ctx, g, [0], 0, False, bufs, count=-1)
    with pytest.raises(A._l.VglHipError, match="NULL"):
        raw_run(ctx, g, [0], 0, False, [None] * 5)
    with pytest.raises(A._l.VglHipError, match="incoming CSR"):
        no_in.prepare_msbfs("in")
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        sh.prepare_msbfs()
    st = raw_run(ctx, g, [], 0, False, bufs)                               # count == 0 succeeds and writes nothing
    assert st.sources == 0 and st.batches == 0 and untouched()
    st = raw_run(ctx, no_in, [0, 1], 0, False, bufs)                       # direction 0 without an incoming CSR: push only
    assert st.sources == 2 and st.levels_pull == 0 and not any(bool((b == 7).all()) for b in bufs)
    only = torch.full((2,), 7, dtype=torch.int32, device=ctx.device)
    st = raw_run(ctx, no_in, [0, 1], 1, True, [None, None, only, None, None])      # vouched for; one output is enough
    assert st.sources == 2 and bool((only != 7).all())
    for h in (sh, no_in, g):
        h.close()


def test_derived_centralities_against_networkx(ctx):
    nx = pytest.importorskip("networkx")
    A = api()
    V = 200
    rng = np.random.default_rng(31)
    src, dst = rng.integers(0, V, 900), rng.integers(0, V, 900)
    G = nx.DiGraph()
    G.add_nodes_from(range(V))
    G.add_edges_from(zip(src.tolist(), dst.tolist()))
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber="total")
    bound = V * 2.0 ** -52
    ref = R.multi_source_bfs(V, src, dst, range(V), "in", want_levels=False)
    for wf in (True, False):
        got, _ = A.closeness_centrality(g, wf_improved=wf)
        assert got.dtype == torch.float64 and same_bits(got.cpu().numpy(), R.closeness(ref, V, wf))
        want = nx.closeness_centrality(G, wf_improved=wf)
        err = max(abs(float(got[v]) - want[v]) / want[v] if want[v] > 0 else abs(float(got[v])) for v in range(V))
        print("closeness wf_improved", wf, "largest relative error", err, "bound", bound)
        assert err <= bound
    got, _ = A.harmonic_centrality(g)
    want = nx.harmonic_centrality(G)
    err = max(abs(float(got[v]) - want[v]) / want[v] if want[v] > 0 else abs(float(got[v])) for v in range(V))
    print("harmonic largest relative error", err, "bound", bound)
    assert err <= bound and same_bits(got.cpu().numpy(), ref["harmonic"])
    some, _ = A.closeness_centrality(g, sources=[5, 199, 5])
    full, _ = A.closeness_centrality(g)
    assert torch.equal(some, full[[5, 199, 5]])
    g.close()


def test_eccentricity_on_a_grid(ctx):
    A = api()
    n = 23
    idx = np.arange(n * n).reshape(n, n)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    g = A.Graph.from_coo(ctx, n * n, *coo(ctx, np.concatenate([a, b]), np.concatenate([b, a])), with_incoming=False)
    ecc, st = A.eccentricity(g, symmetric=True)
    far = np.maximum(np.arange(n), n - 1 - np.arange(n))
    assert ecc.dtype == torch.int32 and np.array_equal(ecc.cpu().numpy().reshape(n, n), np.add.outer(far, far))
    assert st["max_depth"] == 2 * (n - 1) and st["batches"] == -(-n * n // 64)
    g.close()


RECORD = np.dtype([("reached", "<i8"), ("dist_sum", "<i8"), ("ecc", "<i4"), ("pad", "<i4"), ("harmonic", "<f8")])


@pytest.mark.parametrize("fmt", ["csr", "vcsr"])
@pytest.mark.parametrize("incoming", [False, True])
def test_closeness_app(fmt, incoming, ctx, tmp_path):
    """closeness_hip -check against its own sequential BFS, and its -dump against api.multi_source_bfs on the same generated graph"""
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 1)                                     # the app's generator and default seed
    s_np = src.cpu().numpy().astype(np.int64)
    sources = np.flatnonzero(np.bincount(s_np, minlength=V) > 0)[:130].tolist()
    g = A.Graph.from_coo(ctx, V, src, dst)
    want, _ = A.multi_source_bfs(g, sources, direction="in" if incoming else "out")
    g.close()
    dump = str(tmp_path / "dump.bin")
    cmd = [os.path.join(ROOT, "apps", "bin", "closeness_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-sources", "130", "-check", "-format", fmt, "-dump", dump]
    out = subprocess.run(cmd + (["-in"] if incoming else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    assert "error count: 0" in out.stdout and "AVG_PERF" in out.stdout, out.stdout
    got = np.fromfile(dump, RECORD)
    assert got.size == len(sources) and RECORD.itemsize == 32
    for k in KEYS:
        assert same_bits(got[k], want[k].cpu().numpy()), (fmt, incoming, k)
