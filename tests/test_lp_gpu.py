"""Label propagation on the GPU (vgl_hip_lp_run, api.label_propagation, apps/bin/lp_hip) against the numpy restatement of the contract
(tests/lp_reference.py): labels, iteration counts and changed histories are exact, in every mode, direction and numbering."""
import os
import subprocess

import numpy as np
import pytest
import torch

import lp_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def coo(ctx, src, dst):
    return (torch.tensor(np.asarray(src, dtype=np.int32), device=ctx.device), torch.tensor(np.asarray(dst, dtype=np.int32), device=ctx.device))


def host_csr(g, direction):
    rp, adj = (g.out_rowptr, g.out_adj) if direction == "out" else (g.in_rowptr, g.in_adj)
    return rp.cpu().numpy(), adj.cpu().numpy()


MODES = ("ALL_ACTIVE", "FRONTIER", "AUTO")


def run_all_modes(g, **kw):
    A = api()
    res = {}
    for m in MODES:
        labels, st = A.label_propagation(g, mode=getattr(A, "LP_" + m), **kw)
        res[m] = (labels.cpu().numpy(), st)
    return res


def assert_same(res, want):
    labels, its, hist = want
    for m, (got, st) in res.items():
        assert np.array_equal(got, labels), m
        assert st["iterations"] == its and st["changed_history"] == hist, (m, st)
        assert st["converged"] == int(hist[-1] == 0 if hist else 0), (m, st)


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
@pytest.mark.parametrize("direction", ["out", "in"])
def test_hand_cases(name, direction, ctx):
    V, edges, init, max_it, want, iterations, history = R.HAND_CASES[name]
    src, dst = zip(*edges)
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    ref = R.label_propagation(*host_csr(g, direction), init, max_it)
    if direction == "out":
        assert ref[0].tolist() == want and ref[1] == iterations and ref[2] == history
    res = run_all_modes(g, max_iterations=max_it, direction=direction, labels=init)
    assert_same(res, ref)
    g.close()


GRAPHS = [("rmat", 10, 16, 1), ("rmat", 12, 16, 2), ("rmat", 14, 16, 3), ("rmat", 16, 16, 4), ("uniform", 12, 16, 5), ("uniform", 16, 16, 6)]


@pytest.mark.parametrize("kind,scale,ef,seed", GRAPHS)
def test_generated_graphs(kind, scale, ef, seed, ctx):
    A = api()
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    g = A.Graph.from_coo(ctx, V, src, dst)
    for direction in ("out", "in"):
        ref = R.label_propagation(*host_csr(g, direction))
        assert_same(run_all_modes(g, direction=direction), ref)
    g.close()
    s = A.Graph.from_coo(ctx, V, torch.cat([src, dst]), torch.cat([dst, src]), with_incoming=False)
    ref = R.label_propagation(*host_csr(s, "out"))
    res = run_all_modes(s, symmetric=True)
    assert_same(res, ref)
    with pytest.raises(A._l.VglHipError):
        A.label_propagation(s, mode=A.LP_FRONTIER)                   # no incoming CSR and no symmetry vouched for
    s.close()


def test_renumbering_gives_original_order_labels(ctx):
    A = api()
    scale, V = 12, 1 << 12
    src, dst = ctx.gen_rmat(scale, 16, 7)
    base = A.Graph.from_coo(ctx, V, src, dst)
    ref = R.label_propagation(*host_csr(base, "out"))
    for renumber in (None, "out", "total"):
        g = A.Graph.from_coo(ctx, V, src, dst, renumber=renumber)
        for m in MODES:
            labels, st = A.label_propagation(g, mode=getattr(A, "LP_" + m))
            assert np.array_equal(labels.cpu().numpy(), ref[0]), (renumber, m)
            assert st["changed_history"] == ref[2]
        start = torch.arange(V, dtype=torch.int32, device=ctx.device) * 3 - 5000      # explicit start labels, original order
        labels, _ = A.label_propagation(g, labels=start, max_iterations=4)
        assert np.array_equal(labels.cpu().numpy(), R.label_propagation(*host_csr(base, "out"), start.cpu().numpy(), 4)[0]), renumber
        g.close()
    base.close()


CLASSES = ("lp_light", "lp_table64", "lp_table1k", "lp_hubs")


def test_every_class_with_shrunk_thresholds(ctx, monkeypatch):
    A = api()
    for k, v in {"VGL_LP_LIGHT": "4", "VGL_LP_WAVE": "8", "VGL_LP_MEDIUM": "16", "VGL_LP_HUB_CHUNK": "64", "VGL_LP_HUB_SCRATCH_KB": "4",
                 "VGL_LP_PUSH_BIG": "16", "VGL_LP_FRONTIER_SHARE": "0.5"}.items():
        monkeypatch.setenv(k, v)
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 11)
    g = A.Graph.from_coo(ctx, V, src, dst)
    for direction in ("out", "in"):
        ref = R.label_propagation(*host_csr(g, direction))
        ctx.timing(True)
        res = run_all_modes(g, direction=direction)
        launches = {n: ctx.timing_get(n)[0] for n in CLASSES + ("lp_push",)}
        ctx.timing(False)
        assert_same(res, ref)
        assert all(launches[n] > 0 for n in CLASSES + ("lp_push",)), launches
        assert res["FRONTIER"][1]["frontier_steps"] > 0
    g.close()


def hub_graph():
    """two hubs over leaves of their own: hub 0 (200 000 entries, ~200 000 distinct labels) where label 7 leads label 9 by one count, hub 1
    (100 000 entries) where labels -5 and 11 tie at the top (11 wins); the entries are shuffled so that every chunk sees a few of each"""
    rng = np.random.default_rng(5)
    n0, n1 = 200_000, 100_000
    V = 2 + n0 + n1
    init = (np.arange(V, dtype=np.int64) + 1_000_000).astype(np.int32)
    leaves0, leaves1 = 2 + np.arange(n0), 2 + n0 + np.arange(n1)
    init[leaves0[:50]] = 7
    init[leaves0[50:99]] = 9
    init[leaves1[:40]] = -5
    init[leaves1[40:80]] = 11
    src = np.concatenate([np.zeros(n0, np.int64), np.ones(n1, np.int64)])
    dst = np.concatenate([rng.permutation(leaves0), rng.permutation(leaves1)])
    return V, src, dst, init


@pytest.mark.parametrize("scratch_kb", [None, "1024"])
def test_hubs_beyond_any_lds_table(scratch_kb, ctx, monkeypatch):
    A = api()
    if scratch_kb:
        monkeypatch.setenv("VGL_LP_HUB_SCRATCH_KB", scratch_kb)           # smaller than hub 0's table: it raises the cap for itself
    V, src, dst, init = hub_graph()
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    ref = R.label_propagation(*host_csr(g, "out"), init, 3)
    assert ref[0][0] == 7 and ref[0][1] == 11
    res = run_all_modes(g, labels=init, max_iterations=3)
    assert_same(res, ref)
    g.close()


def test_zero_iterations_determinism_and_counts(ctx):
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 13)
    g = A.Graph.from_coo(ctx, V, src, dst)
    start = torch.randint(-100, 100, (V,), dtype=torch.int32, device=ctx.device)
    labels, st = A.label_propagation(g, max_iterations=0, labels=start)
    assert torch.equal(labels, start) and st["iterations"] == 0 and st["changed_history"] == []
    a, sa = A.label_propagation(g, mode=A.LP_AUTO)
    b, sb = A.label_propagation(g, mode=A.LP_AUTO)
    assert torch.equal(a, b) and sa == sb
    _, s = A.label_propagation(g, mode=A.LP_ALL_ACTIVE)
    assert s["edges_examined"] == s["iterations"] * g.E and s["frontier_steps"] == 0
    g.prepare_label_propagation("in")
    g.close()


def test_errors(ctx):
    A = api()
    V = 1 << 10
    src, dst = ctx.gen_rmat(10, 8, 17)
    g = A.Graph.from_coo(ctx, V, src, dst)
    sh = g.shard(0, V // 2)
    out_only = A.Graph.from_coo(ctx, V, src, dst, with_incoming=False)
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        A.label_propagation(sh)
    with pytest.raises(A._l.VglHipError, match="incoming CSR"):
        A.label_propagation(out_only, direction="in")
    with pytest.raises(A._l.VglHipError, match="FRONTIER"):
        A.label_propagation(out_only, mode=A.LP_FRONTIER)
    with pytest.raises(A._l.VglHipError, match="max_iterations"):
        A.label_propagation(g, max_iterations=-1)
    _, st = A.label_propagation(out_only, mode=A.LP_AUTO)                # AUTO without a reverse CSR: every row every iteration
    assert st["frontier_steps"] == 0
    for h in (sh, out_only, g):
        h.close()


def test_lp_app(tmp_path):
    dumps = []
    for fmt in ("csr", "vcsr"):
        dump = str(tmp_path / (fmt + ".bin"))
        cmd = [os.path.join(ROOT, "apps", "bin", "lp_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-check", "-format", fmt, "-dump", dump]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "error count: 0" in out.stdout and "AVG_PERF" in out.stdout, out.stdout
        dumps.append(np.fromfile(dump, np.int32))
    assert dumps[0].size == 1 << 12 and np.array_equal(dumps[0], dumps[1])
