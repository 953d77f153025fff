"""k-truss decomposition on the GPU (vgl_hip_ktruss_run, api.truss_numbers, api.k_truss, apps/bin/ktruss_hip) against the numpy / scipy restatement of
the contract (tests/ktruss_reference.py) and closed forms.  Edges, truss numbers, supports and the statistics are integers: everything is exact
equality."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import ktruss_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = ("ktruss_classify", "ktruss_sup_short", "ktruss_sup_wave", "ktruss_sup_wg", "ktruss_scan", "ktruss_short", "ktruss_wave", "ktruss_wg", "ktruss_publish")
INT_STATS = ("max_truss", "rounds", "max_support", "sub_rounds", "undirected_edges", "triangles", "support_elements", "peel_elements", "algorithmic_bytes")
_REFS = {}


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def coo(ctx, src, dst):
    return (torch.tensor(np.asarray(src, dtype=np.int32), device=ctx.device), torch.tensor(np.asarray(dst, dtype=np.int32), device=ctx.device))


def generated(ctx, kind, scale, ef, seed):
    """(src, dst, the one reference result) of a generated graph: computed once, shared, left unchanged"""
    key = (kind, scale, ef, seed)
    if key not in _REFS:
        src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
        _REFS[key] = (src, dst, R.truss_numbers(1 << scale, src.cpu().numpy(), dst.cpu().numpy()))
    return _REFS[key]


def assert_equals_reference(g, ref, what, **kw):
    """edges, truss, support and the exact statistics of one full run against the one reference result"""
    eu, ev, truss, support, triangles, rounds, sub_rounds = ref
    top, st = api().truss_numbers(g, support=True, **kw)
    print(what, {k: v for k, v in st.items() if not torch.is_tensor(v)})
    assert st["edges"].dtype == st["truss"].dtype == st["support"].dtype == torch.int32, what
    assert tuple(st["edges"].shape) == (eu.size, 2) and np.array_equal(st["edges"].cpu().numpy(), np.stack([eu, ev], axis=1)), what
    assert np.array_equal(st["truss"].cpu().numpy(), truss), what
    assert np.array_equal(st["support"].cpu().numpy(), support), what
    assert top == st["max_truss"] == (int(truss.max()) if truss.size else 0), what
    assert st["rounds"] == rounds and st["sub_rounds"] == sub_rounds, (what, st["rounds"], rounds, st["sub_rounds"], sub_rounds)
    assert st["triangles"] == triangles and st["undirected_edges"] == eu.size, what
    assert st["max_support"] == (int(support.max()) if support.size else 0), what
    assert st["support_elements"] == st["peel_elements"], what                   # a full peel expands every edge once
    assert st["algorithmic_bytes"] == 28 * eu.size + 4 * (st["support_elements"] + st["peel_elements"]), what
    return st


def launches(ctx):
    return {n: ctx.timing_get(n)[0] for n in SLOTS}


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
@pytest.mark.parametrize("renumber", [None, "total"])
def test_hand_cases(name, renumber, ctx):
    V, edges, want = R.HAND_CASES[name]
    src, dst = [a for a, _ in edges], [b for _, b in edges]
    ref = R.truss_numbers(V, src, dst)
    assert ref[2].tolist() == want
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber=renumber)
    assert_equals_reference(g, ref, name)
    g.close()


GRAPHS = [("rmat", 10, 16, 1), ("rmat", 10, 64, 2), ("rmat", 12, 16, 3), ("uniform", 12, 16, 5)]


@pytest.mark.parametrize("kind,scale,ef,seed", GRAPHS)
def test_generated_graphs(kind, scale, ef, seed, ctx):
    """the directed graph, the symmetrised graph (no incoming CSR) and the renumbered graph: one reference result"""
    A = api()
    V = 1 << scale
    src, dst, ref = generated(ctx, kind, scale, ef, seed)
    g = A.Graph.from_coo(ctx, V, src, dst)
    st = assert_equals_reference(g, ref, "directed")
    assert st["triangles"] == A.triangle_count(g)[0]
    deg = np.bincount(np.concatenate([ref[0], ref[1]]), minlength=V)
    assert st["support_elements"] == int(np.minimum(deg[ref[0]], deg[ref[1]]).sum())      # the shorter row of every edge, walked once
    g.close()
    s = A.Graph.from_coo(ctx, V, torch.cat([src, dst]), torch.cat([dst, src]), with_incoming=False)
    assert_equals_reference(s, ref, "symmetrised")
    s.close()
    r = A.Graph.from_coo(ctx, V, src, dst, renumber="total")
    assert_equals_reference(r, ref, "renumbered")
    top, raw = A.truss_numbers(r, support=True, raw=True)                        # the graph's own numbering and edge order
    bwd = r.bwd.cpu().numpy().astype(np.int64)
    e = raw["edges"].cpu().numpy().astype(np.int64)
    assert bool((e[:, 0] < e[:, 1]).all()) and bool((np.diff(e[:, 0] * V + e[:, 1]) > 0).all())
    a, b = bwd[e[:, 0]], bwd[e[:, 1]]
    key = np.minimum(a, b) * V + np.maximum(a, b)
    at = np.searchsorted(ref[0].astype(np.int64) * V + ref[1], key)              # every raw edge is one of the reference's, in ORIGINAL ids
    assert np.unique(key).size == ref[0].size and np.array_equal(ref[0].astype(np.int64)[at] * V + ref[1][at], key)
    assert top == int(ref[2].max()) and np.array_equal(raw["truss"].cpu().numpy(), ref[2][at]) and np.array_equal(raw["support"].cpu().numpy(), ref[3][at])
    r.close()


SHRUNK = {"VGL_KTRUSS_SHORT": "2", "VGL_KTRUSS_WAVE": "8"}


def test_every_class_with_shrunk_thresholds(ctx, monkeypatch):
    A = api()
    V = 1 << 12
    src, dst, ref = generated(ctx, "rmat", 12, 16, 3)
    g = A.Graph.from_coo(ctx, V, torch.cat([src, dst]), torch.cat([dst, src]), with_incoming=False)
    ctx.timing(True)
    st0 = assert_equals_reference(g, ref, "default thresholds")
    n0 = launches(ctx)
    assert st0["prepared_now"] == 1
    for k, v in SHRUNK.items():
        monkeypatch.setenv(k, v)
    ctx.timing(True)
    st1 = assert_equals_reference(g, ref, "shrunk thresholds, cached prepare")
    n1 = launches(ctx)
    ctx.timing(False)
    print("launches under the default / shrunk thresholds", n0, n1)
    assert st1["prepared_now"] == 0
    assert all(n1[k] > 0 for k in SLOTS), n1
    assert n0["ktruss_sup_short"] == 1 and n0["ktruss_short"] >= 1, n0
    assert torch.equal(st0["truss"], st1["truss"]) and torch.equal(st0["support"], st1["support"]) and torch.equal(st0["edges"], st1["edges"])
    assert all(st0[k] == st1[k] for k in INT_STATS), (st0, st1)
    g.close()


@pytest.mark.parametrize("first", ["kcore", "ktruss", "msf"])
def test_kcore_and_ktruss_share_the_symmetric_csr(first, ctx):
    """kcore, ktruss and msf on one handle, each of them first once: the symmetric CSR is built once, and prepared_now is 1 only for the caller
    that built its own stage (kcore: the CSR, ktruss: the edge numbering, msf: the edge of every stored entry)"""
    import kcore_reference as KR
    import msf_reference as MR
    A = api()
    V = 1 << 10
    src, dst, ref = generated(ctx, "rmat", 10, 16, 1)
    core = KR.core_numbers(V, src.cpu().numpy(), dst.cpu().numpy())
    w = ctx.gen_weights(src.numel(), 1)
    forest = MR.minimum_spanning_forest(V, src.cpu().numpy(), dst.cpu().numpy(), w.cpu().numpy())
    g = A.Graph.from_coo(ctx, V, src, dst, want_perm=True)
    w_csr = ctx.gather_u32(g.perm, w)
    ctx.timing(True)
    if first == "kcore":
        _, kc = A.core_numbers(g, degree=True)
        kt = assert_equals_reference(g, ref, "after kcore")
        assert kc["prepared_now"] == 1 and kt["prepared_now"] == 1              # each built what is its own: the CSR / the edge numbering
        _, ms = A.minimum_spanning_forest(g, w_csr, component=True, raw=True)
        assert ms["prepared_now"] == 1                                           # ... / the edge of every stored entry
    elif first == "ktruss":
        kt = assert_equals_reference(g, ref, "before kcore")
        _, kc = A.core_numbers(g, degree=True)
        assert kt["prepared_now"] == 1 and kc["prepared_now"] == 0
        _, ms = A.minimum_spanning_forest(g, w_csr, component=True, raw=True)
        assert ms["prepared_now"] == 1
    else:
        _, ms = A.minimum_spanning_forest(g, w_csr, component=True, raw=True)
        kt = assert_equals_reference(g, ref, "after msf")
        _, kc = A.core_numbers(g, degree=True)
        assert ms["prepared_now"] == 1 and kt["prepared_now"] == 0 and kc["prepared_now"] == 0      # msf built all three stages
    built = ctx.timing_get("kcore_csr")[0]
    ctx.timing(False)
    assert built == 1, built                                                     # the symmetric CSR was built once for the three of them
    assert np.array_equal(kc["core"].cpu().numpy(), core[0]) and np.array_equal(kc["degree"].cpu().numpy(), core[1])
    assert kc["undirected_edges"] == kt["undirected_edges"] == core[2]
    assert ms["undirected_edges"] == core[2] and ms["forest_edges"] == forest["forest_edges"] and ms["rounds"] == forest["rounds"]
    assert np.array_equal(ms["all_edges"].cpu().numpy(), np.stack([forest["edge_u"], forest["edge_v"]], axis=1))
    assert np.array_equal(ms["edge_weight"].cpu().numpy(), forest["edge_w"]) and np.array_equal(ms["in_forest"].cpu().numpy(), forest["forest"])
    assert np.array_equal(ms["component"].cpu().numpy(), forest["component"])
    g.close()


def test_book_contention_on_the_spine(ctx):
    """100 000 pages decrement one address, the spine's support; it crosses k - 1 -> k - 2 once, when the last page edge has been expanded"""
    A = api()
    n = 100_000
    V, src, dst = R.book(n)
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst), with_incoming=False)
    ctx.timing(True)
    top, st = A.truss_numbers(g, support=True)
    n_launch = launches(ctx)
    ctx.timing(False)
    print("book", {k: v for k, v in st.items() if not torch.is_tensor(v)}, n_launch)
    assert top == 3 and bool((st["truss"] == 3).all())
    assert st["edges"][0].tolist() == [0, 1] and int(st["support"][0]) == n and bool((st["support"][1:] == 1).all())
    assert st["max_support"] == n and st["rounds"] == 1 and st["sub_rounds"] == 2
    assert st["triangles"] == n and st["undirected_edges"] == 2 * n + 1
    assert st["support_elements"] == st["peel_elements"] == (n + 1) + 2 * (2 * n)      # the spine walks a row of n + 1, each of the 2 n page edges a row of 2
    assert n_launch["ktruss_sup_wg"] == 1 and n_launch["ktruss_wg"] == 1, n_launch      # both rows of the spine are in the longest class
    g.close()


def test_clique_200_no_decrement_lands(ctx):
    """K_200: every edge is in the first frontier; all three edges of every triangle are in it, so no decrement may land"""
    A = api()
    n = 200
    iu = torch.triu_indices(n, n, offset=1, device=ctx.device).to(torch.int32)
    g = A.Graph.from_coo(ctx, n, iu[0].contiguous(), iu[1].contiguous(), with_incoming=False)
    top, st = A.truss_numbers(g, support=True)
    print("K_200", {k: v for k, v in st.items() if not torch.is_tensor(v)})
    assert top == n and bool((st["truss"] == n).all()) and bool((st["support"] == n - 2).all())
    assert st["rounds"] == 1 and st["sub_rounds"] == 1 and st["triangles"] == math.comb(n, 3) and st["undirected_edges"] == math.comb(n, 2)
    assert torch.equal(st["edges"], iu.t().contiguous())
    g.close()


def test_complete_tripartite_64(ctx):
    A = api()
    m = 64
    V, src, dst = R.tripartite(m)
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    top, st = A.truss_numbers(g, support=True)
    print("K_64,64,64", {k: v for k, v in st.items() if not torch.is_tensor(v)})
    assert top == m + 2 and bool((st["truss"] == m + 2).all()) and bool((st["support"] == m).all())
    assert st["rounds"] == 1 and st["sub_rounds"] == 1 and st["triangles"] == m ** 3 and st["undirected_edges"] == 3 * m * m
    g.close()


@pytest.mark.parametrize("capped_both", [True, False])
def test_tube(capped_both, ctx):
    """capped at both ends: every edge in two triangles, one sub-round; one end open: the long tail of 4 - 8-edge frontiers, two sub-rounds per ring"""
    A = api()
    V, src, dst = R.tube(1024, capped_both)
    ref = R.truss_numbers(V, src, dst)
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    st = assert_equals_reference(g, ref, "tube, capped_both=%s" % capped_both)
    if capped_both:
        assert bool((st["truss"] == 4).all()) and bool((st["support"] == 2).all()) and st["rounds"] == 1 and st["sub_rounds"] == 1
    else:
        assert bool((st["truss"] == 3).all()) and st["rounds"] == 1 and st["sub_rounds"] == ref[6] == 2048
    g.close()


def test_k_limit_and_k_truss(ctx):
    A = api()
    V = 1 << 12
    src, dst, ref = generated(ctx, "rmat", 12, 16, 3)
    eu, ev, truss = ref[0], ref[1], ref[2]
    top = int(truss.max())
    assert top >= 5
    g = A.Graph.from_coo(ctx, V, src, dst, renumber="total")
    for k_limit in (2, 3, top, top + 5):
        want = R.truss_numbers(V, src.cpu().numpy(), dst.cpu().numpy(), k_limit)
        got, st = A.truss_numbers(g, k_limit=k_limit, support=True)
        assert np.array_equal(want[2], np.minimum(truss, k_limit)) and np.array_equal(st["truss"].cpu().numpy(), want[2]), k_limit
        assert np.array_equal(st["support"].cpu().numpy(), ref[3]) and st["triangles"] == ref[4], k_limit
        assert got == st["max_truss"] == min(top, k_limit), k_limit
        assert st["rounds"] == want[5] and st["sub_rounds"] == want[6], (k_limit, st["rounds"], want[5], st["sub_rounds"], want[6])
        member = A.k_truss(g, k_limit)
        keep = truss >= k_limit
        assert member.dtype == torch.int32 and np.array_equal(member.cpu().numpy(), np.stack([eu[keep], ev[keep]], axis=1)), k_limit
    g.close()


def test_two_runs_agree_and_prepare_is_cached(ctx):
    A = api()
    V = 1 << 12
    src, dst, ref = generated(ctx, "rmat", 12, 16, 3)
    g = A.Graph.from_coo(ctx, V, src, dst)
    _, s0 = A.truss_numbers(g, support=True)
    _, s1 = A.truss_numbers(g, support=True)
    assert s0["prepared_now"] == 1 and s1["prepared_now"] == 0
    assert all(torch.equal(s0[k], s1[k]) for k in ("edges", "truss", "support"))
    assert all(s0[k] == s1[k] for k in INT_STATS), (s0, s1)
    assert np.array_equal(s0["truss"].cpu().numpy(), ref[2])
    g.close()
    p = A.Graph.from_coo(ctx, V, src, dst)
    assert p.prepare_ktruss() == ref[0].size
    _, s2 = A.truss_numbers(p)
    assert s2["prepared_now"] == 0 and torch.equal(s2["truss"], s0["truss"]) and "support" not in s2
    p.close()


def test_errors(ctx):
    A = api()
    V = 1 << 10
    src, dst, ref = generated(ctx, "rmat", 10, 16, 1)
    g = A.Graph.from_coo(ctx, V, src, dst)
    sh = g.shard(0, V // 2)
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        A.truss_numbers(sh)
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        sh.prepare_ktruss()
    n = ref[0].size
    buf = [ctx.empty(n, torch.int32) for _ in range(3)]
    ptr = [A._ptr(b) for b in buf]
    with pytest.raises(A._l.VglHipError, match="d_truss"):
        A._l.check(ctx.L.vgl_hip_ktruss_run(ctx.h, g.h, 0, None, None, None, None, None))
    with pytest.raises(A._l.VglHipError, match="d_edge_u and d_edge_v"):
        A._l.check(ctx.L.vgl_hip_ktruss_run(ctx.h, g.h, 0, ptr[0], None, ptr[2], None, None))
    with pytest.raises(A._l.VglHipError, match="d_edge_u and d_edge_v"):
        A._l.check(ctx.L.vgl_hip_ktruss_run(ctx.h, g.h, 0, None, ptr[1], ptr[2], None, None))
    for bad in (1, -1):
        with pytest.raises(A._l.VglHipError, match="k_limit"):
            A.truss_numbers(g, k_limit=bad)
    with pytest.raises(A._l.VglHipError, match="at least 2"):
        A.k_truss(g, 1)
    A._l.check(ctx.L.vgl_hip_ktruss_run(ctx.h, g.h, 0, None, None, ptr[2], None, None))      # the endpoint arrays are optional
    assert np.array_equal(buf[2].cpu().numpy(), ref[2])
    for h in (sh, g):
        h.close()


def test_ktruss_app(tmp_path, ctx):
    dumps = []
    for fmt in ("csr", "vcsr"):
        dump = str(tmp_path / (fmt + ".bin"))
        cmd = [os.path.join(ROOT, "apps", "bin", "ktruss_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-check", "-format", fmt, "-dump", dump]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "error count: 0" in out.stdout and "AVG_PERF" in out.stdout, out.stdout
        assert "error count" not in out.stdout.replace("error count: 0", ""), out.stdout
        dumps.append(np.fromfile(dump, np.int32))
    assert np.array_equal(dumps[0], dumps[1])
    src, dst = ctx.gen_rmat(12, 16, 1)                                           # what -gen generates: the app's default seed, the same generator
    ref = R.truss_numbers(1 << 12, src.cpu().numpy(), dst.cpu().numpy())
    assert np.array_equal(dumps[0].reshape(-1, 3), np.stack([ref[0], ref[1], ref[2]], axis=1))
