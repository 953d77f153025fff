"""Minimum spanning forest on the GPU (vgl_hip_msf_run, api.minimum_spanning_forest, apps/bin/msf_hip) against the numpy restatement of the contract
(tests/msf_reference.py).  The forest mask, the folded weights, the components and the statistics are compared by exact equality; total_weight exactly
for integer-valued weights and within the first-order bound of a float64 sum otherwise."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import msf_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = ("msf_prepare", "msf_fold", "msf_min_short", "msf_min_wave", "msf_min_wg", "msf_hook", "msf_flatten", "msf_publish")
INT_STATS = ("rounds", "forest_edges", "components", "undirected_edges", "entries_walked", "algorithmic_bytes")
_REFS = {}


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def dev(ctx, a, dtype):
    return torch.tensor(np.asarray(a, dtype=dtype), device=ctx.device)


def csr_weights(ctx, g, w):
    """the weights of the COO entries (a device float32 tensor) in the order of the graph's outgoing CSR"""
    return ctx.gather_u32(g.perm, w) if w.numel() else w


def assert_equals_reference(g, w_csr, ref, what):
    """one run with raw=True against the restatement on the graph's own numbering: every edge, folded weight, the mask, the components, the statistics"""
    total, st = api().minimum_spanning_forest(g, w_csr, component=True, raw=True)
    print(what, {k: v for k, v in st.items() if not torch.is_tensor(v)})
    n = ref["undirected_edges"]
    assert st["all_edges"].dtype == st["component"].dtype == torch.int32 and st["edge_weight"].dtype == torch.float32, what
    assert tuple(st["all_edges"].shape) == (n, 2) and np.array_equal(st["all_edges"].cpu().numpy(), np.stack([ref["edge_u"], ref["edge_v"]], axis=1)), what
    got_w = st["edge_weight"].cpu().numpy()
    assert np.array_equal(got_w, ref["edge_w"]) and np.array_equal(np.signbit(got_w), np.signbit(ref["edge_w"])), what
    assert np.array_equal(st["in_forest"].cpu().numpy(), ref["forest"]), what
    assert np.array_equal(st["edges"].cpu().numpy(), np.stack([ref["edge_u"], ref["edge_v"]], axis=1)[ref["forest"]]), what
    assert np.array_equal(st["weights"].cpu().numpy(), ref["edge_w"][ref["forest"]]), what
    assert np.array_equal(st["component"].cpu().numpy(), ref["component"]), what
    for k in ("rounds", "forest_edges", "components", "undirected_edges"):
        assert st[k] == ref[k], (what, k, st[k], ref[k])
    if n:
        assert 2 * n <= st["entries_walked"] <= (st["rounds"] + 1) * 2 * n, (what, st["entries_walked"])
    else:
        assert st["entries_walked"] == 0 and st["rounds"] == 0
    assert st["algorithmic_bytes"] == (8 * g.E + 5 * n + 12 * st["entries_walked"] + 20 * g.V * st["rounds"] if n else 0), what      # no edge: no pass runs
    assert_total(total, st, ref, what)
    return st


def assert_total(total, st, ref, what):
    w = ref["edge_w"][ref["forest"]].astype(np.float64)
    assert total == st["total_weight"]
    if bool((w == np.rint(w)).all()) or not np.isfinite(w).all():                # integer-valued (or an infinity): every partial sum is exact
        assert total == ref["total"], (what, total, ref["total"])
    else:                                                                        # any order of n float64 additions, first order, doubled
        bound = w.size * 2.0 ** -52 * math.fsum(np.abs(w).tolist())
        print(what, "total", total, "fsum", ref["total"], "difference", abs(total - ref["total"]), "bound", bound)
        assert abs(total - ref["total"]) <= bound, (what, total, ref["total"], bound)


def launches(ctx):
    return {n: ctx.timing_get(n)[0] for n in SLOTS}


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
@pytest.mark.parametrize("renumber", [None, "total"])
def test_hand_cases(name, renumber, ctx):
    """the renumbered graph breaks ties by ITS numbering: the restatement runs on the COO relabelled by g.fwd"""
    V, src, dst, w, want = R.hand_case(name)
    g = api().Graph.from_coo(ctx, V, dev(ctx, src, np.int32), dev(ctx, dst, np.int32), want_perm=True, renumber=renumber)
    fwd = g.fwd.cpu().numpy().astype(np.int64) if renumber else np.arange(V)
    ref = R.minimum_spanning_forest(V, fwd[src] if src.size else src, fwd[dst] if dst.size else dst, w)
    if not renumber:
        assert sorted(zip(ref["edge_u"][ref["forest"]].tolist(), ref["edge_v"][ref["forest"]].tolist())) == want
    assert_equals_reference(g, csr_weights(ctx, g, dev(ctx, w, np.float32)), ref, name)
    g.close()


GRAPHS = [("rmat", 10, 16, 1), ("rmat", 12, 16, 3), ("rmat", 14, 16, 4), ("uniform", 12, 16, 5)]


def generated(ctx, kind, scale, ef, seed, quantised):
    """(src, dst, w) on the device and the one reference result in ORIGINAL numbering: computed once, shared, left unchanged"""
    key = (kind, scale, ef, seed, quantised)
    if key not in _REFS:
        src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
        w = ctx.gen_weights(src.numel(), seed)
        if quantised:
            w = (w.long() % 3 + 1).float()                                       # {1, 2, 3}: almost every comparison is a tie
        _REFS[key] = (src, dst, w, R.minimum_spanning_forest(1 << scale, src.cpu().numpy(), dst.cpu().numpy(), w.cpu().numpy()))
    return _REFS[key]


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("kind,scale,ef,seed", GRAPHS)
def test_generated_graphs(kind, scale, ef, seed, quantised, ctx):
    """the directed graph, the symmetrised graph (no incoming CSR) and the renumbered graph"""
    A = api()
    V = 1 << scale
    src, dst, w, ref = generated(ctx, kind, scale, ef, seed, quantised)
    g = A.Graph.from_coo(ctx, V, src, dst, want_perm=True)
    assert_equals_reference(g, csr_weights(ctx, g, w), ref, "directed")
    g.close()
    s = A.Graph.from_coo(ctx, V, torch.cat([src, dst]), torch.cat([dst, src]), with_incoming=False, want_perm=True)
    assert_equals_reference(s, csr_weights(ctx, s, torch.cat([w, w])), ref, "symmetrised")
    s.close()
    r = A.Graph.from_coo(ctx, V, src, dst, want_perm=True, renumber="total")
    w_r = csr_weights(ctx, r, w)
    fwd = r.fwd.cpu().numpy().astype(np.int64)
    own = R.minimum_spanning_forest(V, fwd[src.cpu().numpy()], fwd[dst.cpu().numpy()], w.cpu().numpy())      # ties break by the graph's own numbering
    assert_equals_reference(r, w_r, own, "renumbered, raw")
    total, st = A.minimum_spanning_forest(r, w_r, component=True)                # ORIGINAL ids, ascending (lo, hi)
    e = st["all_edges"].cpu().numpy()
    assert np.array_equal(e, np.stack([ref["edge_u"], ref["edge_v"]], axis=1)) and np.array_equal(st["edge_weight"].cpu().numpy(), ref["edge_w"])
    assert np.array_equal(np.sort(st["weights"].cpu().numpy()), np.sort(ref["edge_w"][ref["forest"]]))      # the weights of a minimum forest are unique as a multiset
    assert st["forest_edges"] == ref["forest_edges"] and st["components"] == ref["components"]
    comp = st["component"].cpu().numpy()                                         # the same partition; the representative is a member
    assert np.array_equal(comp[comp], comp)
    pairs = np.unique(np.stack([comp, ref["component"]], axis=1), axis=0)
    assert pairs.shape[0] == np.unique(comp).size == np.unique(ref["component"]).size == ref["components"]
    r.close()


@pytest.mark.parametrize("kind,scale,ef,seed", GRAPHS)
def test_distinct_weights_forest_is_the_same_set_in_any_numbering(kind, scale, ef, seed, ctx):
    """With no two weights equal there is no tie to break, so the forest of the renumbered handle, in ORIGINAL ids, is the original-numbering
    reference's edge for edge.  gen_weights draws from 2^24 values and repeats some at these sizes (test_generated_graphs compares those runs in the
    graph's own numbering), so the weights here are a permutation of 1 .. E: distinct, and exact in float32 (E <= 2^18)."""
    A = api()
    V = 1 << scale
    src, dst, _, _ = generated(ctx, kind, scale, ef, seed, False)
    w_host = np.random.default_rng(seed).permutation(src.numel()).astype(np.float32) + np.float32(1.0)
    ref = R.minimum_spanning_forest(V, src.cpu().numpy(), dst.cpu().numpy(), w_host)
    assert np.unique(ref["edge_w"]).size == ref["edge_w"].size
    r = A.Graph.from_coo(ctx, V, src, dst, want_perm=True, renumber="total")
    total, st = A.minimum_spanning_forest(r, csr_weights(ctx, r, dev(ctx, w_host, np.float32)))
    pairs = np.stack([ref["edge_u"], ref["edge_v"]], axis=1)
    assert np.array_equal(st["all_edges"].cpu().numpy(), pairs) and np.array_equal(st["edge_weight"].cpu().numpy(), ref["edge_w"])
    assert np.array_equal(st["in_forest"].cpu().numpy(), ref["forest"])
    assert np.array_equal(st["edges"].cpu().numpy(), pairs[ref["forest"]])
    assert np.array_equal(st["weights"].cpu().numpy(), ref["edge_w"][ref["forest"]]) and "component" not in st
    assert st["rounds"] == ref["rounds"] and st["forest_edges"] == ref["forest_edges"] and total == ref["total"]
    r.close()


SHRUNK = {"VGL_MSF_SHORT": "2", "VGL_MSF_WAVE": "8", "VGL_MSF_CHUNK": "16"}


def test_every_class_with_shrunk_thresholds(ctx, monkeypatch):
    A = api()
    V = 1 << 12
    src, dst, w, ref = generated(ctx, "rmat", 12, 16, 3, False)
    g = A.Graph.from_coo(ctx, V, src, dst, want_perm=True)
    w_csr = csr_weights(ctx, g, w)
    ctx.timing(True)
    st0 = assert_equals_reference(g, w_csr, ref, "default thresholds")
    n0 = launches(ctx)
    assert st0["prepared_now"] == 1 and n0["msf_prepare"] == 1
    for k, v in SHRUNK.items():
        monkeypatch.setenv(k, v)
    ctx.timing(True)
    st1 = assert_equals_reference(g, w_csr, ref, "shrunk thresholds, cached prepare")
    n1 = launches(ctx)
    ctx.timing(False)
    print("launches under the default / shrunk thresholds", n0, n1)
    assert st1["prepared_now"] == 0 and n1["msf_prepare"] == 0
    assert all(n1[k] > 0 for k in SLOTS if k != "msf_prepare"), n1
    assert n0["msf_min_short"] >= 1 and n0["msf_fold"] == 1, n0
    for k in ("all_edges", "edge_weight", "in_forest", "component"):
        assert torch.equal(st0[k], st1[k]), k
    assert all(st0[k] == st1[k] for k in INT_STATS) and st0["total_weight"] == st1["total_weight"], (st0, st1)
    g.close()


def test_star_100000_leaves_equal_weights(ctx):
    """every leaf and the hub pick in the first round; the hub's row of 100 000 entries goes through the workgroup class"""
    A = api()
    n = 100_000
    V, src, dst, w = R.star(n)
    g = A.Graph.from_coo(ctx, V, dev(ctx, src, np.int32), dev(ctx, dst, np.int32), with_incoming=False, want_perm=True)
    ctx.timing(True)
    total, st = A.minimum_spanning_forest(g, csr_weights(ctx, g, dev(ctx, w, np.float32)), component=True)
    n_launch = launches(ctx)
    ctx.timing(False)
    print("star", {k: v for k, v in st.items() if not torch.is_tensor(v)}, n_launch)
    assert st["rounds"] == 1 and st["forest_edges"] == n and st["components"] == 1 and st["undirected_edges"] == n
    assert bool(st["in_forest"].all()) and bool((st["component"] == 0).all()) and total == float(n)
    assert n_launch["msf_min_wg"] >= 1 and n_launch["msf_min_short"] >= 1, n_launch
    assert 2 * n <= st["entries_walked"] <= 4 * n
    g.close()


def test_ruler_path_the_live_list_shrinks(ctx):
    """>= 10 rounds on the path while the clique's 600 rows are finished after the first: rows that are never dropped would be walked in every round,
    about (rounds + 1) 2 E' entries (13 x 2 E'); with the live list the clique is walked twice"""
    A = api()
    V, src, dst, w = R.ruler(4096, 600)
    ref = R.minimum_spanning_forest(V, src, dst, w)
    assert ref["rounds"] >= 10 and ref["forest_edges"] == V - 1
    g = A.Graph.from_coo(ctx, V, dev(ctx, src, np.int32), dev(ctx, dst, np.int32), with_incoming=False, want_perm=True)
    st = assert_equals_reference(g, csr_weights(ctx, g, dev(ctx, w, np.float32)), ref, "ruler")
    assert st["rounds"] == ref["rounds"]
    print("ruler: entries walked / 2E'", st["entries_walked"] / (2 * ref["undirected_edges"]))
    assert st["entries_walked"] < 3 * 2 * ref["undirected_edges"], (st["entries_walked"], ref["undirected_edges"])
    g.close()


def test_total_weight_and_two_runs_agree(ctx):
    A = api()
    V = 1 << 12
    for quantised in (True, False):
        src, dst, w, ref = generated(ctx, "rmat", 12, 16, 3, quantised)
        g = A.Graph.from_coo(ctx, V, src, dst, want_perm=True)
        assert g.prepare_msf() == ref["undirected_edges"]
        w_csr = csr_weights(ctx, g, w)
        t0, s0 = A.minimum_spanning_forest(g, w_csr, component=True)
        t1, s1 = A.minimum_spanning_forest(g, w_csr, component=True)
        assert s0["prepared_now"] == 0 and s1["prepared_now"] == 0               # prepare_msf() built it
        assert_total(t0, s0, ref, "quantised" if quantised else "generated")
        assert np.float64(t0).tobytes() == np.float64(t1).tobytes()              # bit-equal
        assert all(s0[k] == s1[k] for k in INT_STATS), (s0, s1)
        assert all(torch.equal(s0[k], s1[k]) for k in ("edges", "weights", "in_forest", "component"))
        g.close()


def test_errors(ctx):
    A = api()
    V = 1 << 10
    src, dst, w, ref = generated(ctx, "rmat", 10, 16, 1, False)
    g = A.Graph.from_coo(ctx, V, src, dst, want_perm=True)
    w_csr = csr_weights(ctx, g, w)
    sh = g.shard(0, V // 2)
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        A.minimum_spanning_forest(sh, w_csr)
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        sh.prepare_msf()
    n = ref["undirected_edges"]
    eu, ev = ctx.empty(n, torch.int32), ctx.empty(n, torch.int32)
    mask = torch.full((n,), 7, dtype=torch.uint8, device=ctx.device)
    P, run = A._ptr, ctx.L.vgl_hip_msf_run
    with pytest.raises(A._l.VglHipError, match="d_in_forest"):
        A._l.check(run(ctx.h, g.h, P(w_csr), None, None, None, None, None, None))
    with pytest.raises(A._l.VglHipError, match="d_weights"):
        A._l.check(run(ctx.h, g.h, None, None, None, None, P(mask), None, None))
    with pytest.raises(A._l.VglHipError, match="d_edge_u and d_edge_v"):
        A._l.check(run(ctx.h, g.h, P(w_csr), P(eu), None, None, P(mask), None, None))
    with pytest.raises(A._l.VglHipError, match="d_edge_u and d_edge_v"):
        A._l.check(run(ctx.h, g.h, P(w_csr), None, P(ev), None, P(mask), None, None))
    rows = torch.repeat_interleave(torch.arange(V, device=ctx.device), (g.out_rowptr[1:] - g.out_rowptr[:-1]))
    loops = torch.nonzero(rows == g.out_adj.long()).flatten()
    plain = torch.nonzero(rows != g.out_adj.long()).flatten()
    assert loops.numel() > 0                                                     # RMAT generates some
    bad = w_csr.clone()
    bad[plain[plain.numel() // 2]] = float("nan")
    with pytest.raises(A._l.VglHipError, match="weights"):
        A._l.check(run(ctx.h, g.h, P(bad), None, None, None, P(mask), None, None))
    torch.cuda.synchronize()
    assert bool((mask == 7).all())                                               # reported before any output was written
    ok = w_csr.clone()
    ok[loops] = float("nan")                                                     # a loop's weight is never looked at
    A._l.check(run(ctx.h, g.h, P(ok), None, None, None, P(mask), None, None))    # every other output is optional
    torch.cuda.synchronize()
    assert np.array_equal(mask.cpu().numpy().astype(bool), ref["forest"])
    for h in (sh, g):
        h.close()


def test_msf_app(tmp_path, ctx):
    dumps = []
    for fmt in ("csr", "vcsr"):
        dump = str(tmp_path / (fmt + ".bin"))
        cmd = [os.path.join(ROOT, "apps", "bin", "msf_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-check", "-format", fmt, "-dump", dump]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "error count: 0" in out.stdout and "AVG_PERF" in out.stdout, out.stdout
        assert "error count" not in out.stdout.replace("error count: 0", ""), out.stdout
        dumps.append(np.fromfile(dump, np.int32))
    assert dumps[0].size > 0 and dumps[0].size % 3 == 0
    assert np.array_equal(dumps[0], dumps[1])
    rec = dumps[0].reshape(-1, 3)
    assert bool((rec[:, 0] < rec[:, 1]).all()) and bool((np.diff(rec[:, 0].astype(np.int64) * (1 << 12) + rec[:, 1]) > 0).all())
