"""Betweenness centrality on the GPU (vgl_hip_bc_run, api.betweenness_centrality, apps/bin/bc_hip) against the numpy / scipy restatement of the contract
(tests/bc_reference.py), closed forms and the certificate that needs no reference.  The tolerance is derived, per case from that
case's own D, d_max and S: |got - ref| <= 2 (D (d_max + 4) + S) 2^-53 ref per vertex, exactly 0 where ref is 0.  Levels, path counts below 2^53 and
the integer statistics are compared for equality.  Every comparison prints its largest error as a fraction of its bound."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import bc_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTS = ("sources", "max_depth", "levels_total", "reached_total", "edges_forward", "edges_backward")
SWEEPS = ("short", "wave", "wg", "hub")


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def coo(ctx, src, dst):
    return (torch.tensor(np.asarray(src, dtype=np.int32), device=ctx.device), torch.tensor(np.asarray(dst, dtype=np.int32), device=ctx.device))


def within(got, ref, tol, what):
    ok, frac = R.compare(got, ref, tol)
    print(what, "largest error / bound %.4f" % frac, "(bound %.3e relative)" % tol)
    assert ok, (what, frac)
    return frac


def check_certificate(levels, delta, tol, V, what):
    """sum of the last source's delta over the vertices other than the source against the integer the levels give"""
    want = R.certificate(levels)
    got = float(np.sum(delta[levels != 1]))
    frac = abs(got - want) / ((tol + V * R.U) * max(want, 1))
    print(what, "certificate", got, "expected", want, "error / bound %.4f" % frac)
    assert frac <= 1.0, (what, got, want)


def assert_equals_reference(g, V, src, dst, sources, what, symmetric=False, factor=1.0, exact_sigma=True):
    """bc, the integer statistics and the last source's levels / sigma / delta of one API call against the restatement on the ORIGINAL ids"""
    A = api()
    ref, info = R.betweenness(V, src, dst, sources)
    tol = factor * R.tolerance(info["max_depth"], info["d_max"], info["sources"])
    got, st = A.betweenness_centrality(g, sources, symmetric=symmetric, want_last=True)
    print(what, {k: v for k, v in st.items() if not torch.is_tensor(v)}, "D", info["max_depth"], "d_max", info["d_max"], "sigma max", info["sigma_max"])
    assert got.dtype == torch.float64 and got.numel() == V
    within(got.cpu().numpy(), ref, tol, what + " bc")
    for k in INTS:
        assert st[k] == info[k], (what, k, st[k], info[k])
    levels, sigma, delta = info["last"]
    assert st["levels"].dtype == torch.int32 and np.array_equal(st["levels"].cpu().numpy(), levels), what
    if exact_sigma:
        assert info["sigma_max"] < 2.0 ** 53 and st["sigma_inexact"] == 0
        assert np.array_equal(st["sigma"].cpu().numpy(), sigma), what
    else:
        within(st["sigma"].cpu().numpy(), sigma, tol, what + " sigma")
    within(st["delta"].cpu().numpy(), delta, tol, what + " delta of the last source")
    check_certificate(st["levels"].cpu().numpy(), st["delta"].cpu().numpy(), tol, V, what)
    return got, st, info


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
@pytest.mark.parametrize("renumber", [None, "total"])
def test_hand_cases(name, renumber, ctx):
    V, edges, want = R.HAND_CASES[name]
    src, dst = zip(*edges)
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber=renumber)
    got, _, info = assert_equals_reference(g, V, src, dst, None, name)
    within(got.cpu().numpy(), np.array(want), R.tolerance(info["max_depth"], info["d_max"], V), name + " closed form")
    g.close()


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


GRAPHS = [("rmat", 10, 16, 1), ("rmat", 12, 16, 2), ("rmat", 14, 16, 3), ("rmat", 16, 16, 4), ("uniform", 12, 16, 5), ("uniform", 16, 16, 6)]


@pytest.mark.parametrize("kind,scale,ef,seed", GRAPHS)
def test_generated_graphs(kind, scale, ef, seed, ctx):
    """the directed graph, the symmetrised graph without an incoming CSR (symmetric=True) and the renumbered graph"""
    A = api()
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    s_np, d_np = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
    sources = None if scale == 10 else pick_sources(V, s_np, d_np, 32, seed)
    g = A.Graph.from_coo(ctx, V, src, dst)
    assert_equals_reference(g, V, s_np, d_np, sources, "directed")
    g.close()
    r = A.Graph.from_coo(ctx, V, src, dst, renumber="total")
    got, _, _ = assert_equals_reference(r, V, s_np, d_np, sources, "renumbered")
    raw_sources = [r.vertex_id(s) for s in (range(V) if sources is None else sources)]      # the same sources in the same order: the same bits
    raw, _ = A.betweenness_centrality(r, raw_sources, raw=True)            # the graph's own numbering: original vertex bwd[i] at position i
    assert torch.equal(raw, got[r.bwd.long()])
    r.close()
    both = (torch.cat([src, dst]), torch.cat([dst, src]))
    b_s, b_d = np.concatenate([s_np, d_np]), np.concatenate([d_np, s_np])
    s = A.Graph.from_coo(ctx, V, *both, with_incoming=False)
    sym_sources = None if scale == 10 else pick_sources(V, b_s, b_d, 32, seed)
    got, _, _ = assert_equals_reference(s, V, b_s, b_d, sym_sources, "symmetrised", symmetric=True)
    halved, _ = A.betweenness_centrality(s, sym_sources, symmetric=True, halve=True, rescale=True)
    n = V if sym_sources is None else len(sym_sources)
    assert torch.equal(halved, got * (float(V) / n) * 0.5)
    s.close()


def sweep_launches(ctx, which):
    return {k: ctx.timing_get("bc_%s_%s" % (which, k))[0] for k in SWEEPS}


def test_deep_path_costs_its_entries_not_depth_times_v(ctx):
    """a directed path of 5000 vertices from vertex 0: one launch per level and sweep, 4999 entries walked per sweep -- no per-level pass over all V"""
    A = api()
    n = 5000
    src, dst = np.arange(n - 1), np.arange(1, n)
    g = A.Graph.from_coo(ctx, n, *coo(ctx, src, dst))
    ctx.timing(True)
    got, st, info = assert_equals_reference(g, n, src, dst, [0], "path 5000")
    fwd, bwd, order = sweep_launches(ctx, "forward"), sweep_launches(ctx, "backward"), ctx.timing_get("bc_order")[0]
    ctx.timing(False)
    want = np.array([0.0] + [float(n - 1 - i) for i in range(1, n)])
    assert np.array_equal(got.cpu().numpy(), want)                        # small integers: exact
    assert st["max_depth"] == n - 1 and st["edges_forward"] == n - 1 and st["edges_backward"] == n - 1 and st["reached_total"] == n
    print("launches", fwd, bwd, order)
    assert sum(fwd.values()) == n - 1 and sum(bwd.values()) == n - 1       # one row per level: one launch per level
    assert order <= 8                                                      # count + scatter per direction, whatever the depth
    g.close()


@pytest.mark.parametrize("n,exact", [(29, True), (40, False)])
def test_grid_from_a_corner(n, exact, ctx):
    """n x n grid stored both ways from the corner: sigma[(r, c)] = C(r + c, r); n = 29: the largest is C(56, 28) < 2^53, exact; n = 40: C(78, 39) > 2^53,
    rounded: sigma_inexact = 1 and three times the bound (sigma's own rounding enters coef twice)"""
    A = api()
    assert (math.comb(2 * n - 2, n - 1) < 2 ** 53) == exact
    src, dst = R.grid_both_ways(n)
    g = A.Graph.from_coo(ctx, n * n, *coo(ctx, src, dst))
    got, st, info = assert_equals_reference(g, n * n, src, dst, [0], "grid %d" % n, factor=1.0 if exact else 3.0, exact_sigma=exact)
    assert st["max_depth"] == 2 * (n - 1) and st["sigma_inexact"] == (0 if exact else 1)
    binom = R.grid_sigma(n)
    if exact:
        assert np.array_equal(st["sigma"].cpu().numpy(), binom)
    else:
        within(st["sigma"].cpu().numpy(), binom, 3.0 * R.tolerance(info["max_depth"], info["d_max"], 1), "sigma against the binomials")
    same, _ = A.betweenness_centrality(g, [0], symmetric=True)             # the outgoing CSR serving both sweeps: the same rows, the same bits
    assert torch.equal(same, got)
    g.close()


def test_star_with_a_million_leaves(ctx):
    """centre 0, 2^20 leaves, stored both ways: one row of 2^20 entries in both sweeps (the hub class under the default switches).  From a leaf the centre
    gets k - 1, from the centre nobody gets anything."""
    A = api()
    k = 1 << 20
    leaves = np.arange(1, k + 1)
    src, dst = np.concatenate([np.zeros(k, dtype=np.int64), leaves]), np.concatenate([leaves, np.zeros(k, dtype=np.int64)])
    g = A.Graph.from_coo(ctx, k + 1, *coo(ctx, src, dst))
    ctx.timing(True)
    got, st, _ = assert_equals_reference(g, k + 1, src, dst, [0, 1, 2, k], "star 2^20")
    fwd, bwd = sweep_launches(ctx, "forward"), sweep_launches(ctx, "backward")
    ctx.timing(False)
    assert fwd["hub"] > 0 and bwd["hub"] > 0, (fwd, bwd)
    want = np.zeros(k + 1)
    want[0] = 3.0 * (k - 1)
    assert np.array_equal(got.cpu().numpy(), want)
    g.close()


def test_complete_bipartite_300(ctx):
    """K_{m,m} stored both ways, every vertex a source: a pair on one side has m shortest paths, one through each vertex of the other: m - 1 per vertex"""
    A = api()
    m = 300
    a = np.repeat(np.arange(m), m)
    b = np.tile(np.arange(m, 2 * m), m)
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    g = A.Graph.from_coo(ctx, 2 * m, *coo(ctx, src, dst))
    got, _, info = assert_equals_reference(g, 2 * m, src, dst, None, "K_300,300")
    within(got.cpu().numpy(), np.full(2 * m, float(m - 1)), R.tolerance(info["max_depth"], info["d_max"], 2 * m), "K_300,300 closed form")
    g.close()


SHRUNK = {"VGL_BC_SHORT": "4", "VGL_BC_WAVE": "16", "VGL_BC_WG": "64", "VGL_BC_CHUNK": "16"}


def test_every_row_class_with_shrunk_thresholds(ctx, monkeypatch):
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 11)
    s_np, d_np = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
    b_s, b_d = np.concatenate([s_np, d_np]), np.concatenate([d_np, s_np])
    both = (torch.cat([src, dst]), torch.cat([dst, src]))
    sources = pick_sources(V, b_s, b_d, 32, 11)
    g = A.Graph.from_coo(ctx, V, *both, with_incoming=False)
    first, st, _ = assert_equals_reference(g, V, b_s, b_d, sources, "default thresholds", symmetric=True)
    assert st["prepared_now"] == 1
    g.close()
    for k, v in SHRUNK.items():
        monkeypatch.setenv(k, v)
    g = A.Graph.from_coo(ctx, V, *both, with_incoming=False)              # a new handle under the shrunk switches
    ctx.timing(True)
    _, st, _ = assert_equals_reference(g, V, b_s, b_d, sources, "shrunk thresholds", symmetric=True)
    fwd, bwd = sweep_launches(ctx, "forward"), sweep_launches(ctx, "backward")
    ctx.timing(False)
    print("launches", fwd, bwd)
    assert all(n > 0 for n in fwd.values()) and all(n > 0 for n in bwd.values()), (fwd, bwd)
    d = A.Graph.from_coo(ctx, V, src, dst)                                 # both directions, classes of their own
    assert_equals_reference(d, V, s_np, d_np, pick_sources(V, s_np, d_np, 32, 11), "shrunk thresholds, directed")
    for h in (g, d):
        h.close()


def raw_run(ctx, g, sources, accumulate, buf, symmetric=False):
    A = api()
    n = len(sources)
    arr = (C.c_int32 * max(n, 1))(*sources)
    st = A._l.BcStats()
    A._l.check(ctx.L.vgl_hip_bc_run(ctx.h, g.h, arr, n, int(symmetric), int(accumulate), C.c_void_p(buf.data_ptr()), None, None, None, C.byref(st)))
    ctx.sync()
    return st


def test_reproducible_accumulating_and_overwriting(ctx):
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 13)
    s_np, d_np = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
    g = A.Graph.from_coo(ctx, V, src, dst)
    g.prepare_betweenness()
    sources = pick_sources(V, s_np, d_np, 32, 13)
    one, st1, info = assert_equals_reference(g, V, s_np, d_np, sources, "A + B in one call")
    two, st2 = A.betweenness_centrality(g, sources)
    assert st1["prepared_now"] == 0 and torch.equal(one, two)              # bit-identical
    tol = R.tolerance(info["max_depth"], info["d_max"], len(sources))
    buf = torch.full((V,), float("nan"), dtype=torch.float64, device=ctx.device)
    raw_run(ctx, g, sources[:20], 0, buf)                                  # overwrites the poison
    assert bool(torch.isfinite(buf).all())
    raw_run(ctx, g, sources[20:], 1, buf)                                  # adds to it
    within(buf.cpu().numpy(), one.cpu().numpy(), tol, "accumulate A then B against one call")
    acc = torch.zeros(V, dtype=torch.float64, device=ctx.device)
    out, _ = A.betweenness_centrality(g, sources, bc=acc)
    assert out is acc and torch.equal(acc, one)
    empty = torch.full((V,), float("nan"), dtype=torch.float64, device=ctx.device)
    st = raw_run(ctx, g, [], 0, empty)
    assert st.sources == 0 and bool((empty == 0).all())
    g.close()


def test_errors_leave_the_result_untouched(ctx):
    A = api()
    V = 1 << 10
    src, dst = ctx.gen_rmat(10, 8, 17)
    g = A.Graph.from_coo(ctx, V, src, dst)
    no_in = A.Graph.from_coo(ctx, V, src, dst, with_incoming=False)
    sh = g.shard(0, V // 2)
    buf = torch.full((V,), 7.0, dtype=torch.float64, device=ctx.device)
    cases = [(no_in, [0], False, "incoming CSR"), (g, [0, V], False, "out of range"), (g, [-1], False, "out of range"), (sh, [0], False, "own all rows"),
             (sh, [0], True, "own all rows")]
    for handle, sources, symmetric, message in cases:
        with pytest.raises(A._l.VglHipError, match=message):
            raw_run(ctx, handle, sources, 0, buf, symmetric)
        assert bool((buf == 7.0).all()), message
    with pytest.raises(A._l.VglHipError, match="count"):
        A._l.check(ctx.L.vgl_hip_bc_run(ctx.h, g.h, (C.c_int32 * 1)(0), -1, 0, 0, C.c_void_p(buf.data_ptr()), None, None, None, None))
    with pytest.raises(A._l.VglHipError, match="d_bc"):
        A._l.check(ctx.L.vgl_hip_bc_run(ctx.h, g.h, (C.c_int32 * 1)(0), 1, 0, 0, None, None, None, None, None))
    with pytest.raises(A._l.VglHipError, match="incoming CSR"):
        no_in.prepare_betweenness()
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        sh.prepare_betweenness()
    assert bool((buf == 7.0).all())
    raw_run(ctx, no_in, [0], 0, buf, symmetric=True)                       # vouched for: runs (the answer is that of the stored graph read both ways)
    assert bool((buf != 7.0).all())
    for h in (sh, no_in, g):
        h.close()


def test_bc_app(ctx, tmp_path):
    """bc_hip -check against its own sequential Brandes, and its -dump against api.betweenness_centrality on the same generated graph"""
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 1)                                     # the app's generator and default seed
    s_np, d_np = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
    sources = np.flatnonzero(np.bincount(s_np, minlength=V) > 0)[:16].tolist()
    g = A.Graph.from_coo(ctx, V, src, dst)
    want, _, info = assert_equals_reference(g, V, s_np, d_np, sources, "the app's graph")
    g.close()
    tol = R.tolerance(info["max_depth"], info["d_max"], len(sources))
    for fmt in ("csr", "vcsr"):
        dump = str(tmp_path / (fmt + ".bin"))
        cmd = [os.path.join(ROOT, "apps", "bin", "bc_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-sources", "16", "-check", "-format", fmt, "-dump", dump]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        print(out.stdout)
        assert "error count: 0" in out.stdout and "AVG_PERF" in out.stdout, out.stdout
        assert "error count" not in out.stdout.replace("error count: 0", ""), out.stdout
        got = np.fromfile(dump, np.float64)
        assert got.size == V
        within(got, want.cpu().numpy(), tol, "bc_hip -format " + fmt)
