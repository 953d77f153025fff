"""k-core decomposition on the GPU (vgl_hip_kcore_run, api.core_numbers, api.k_core, apps/bin/kcore_hip) against the numpy / scipy restatement of the
contract (tests/kcore_reference.py) and closed forms.  Core numbers, degrees and the statistics are integers: everything is exact equality."""
import os
import subprocess

import numpy as np
import pytest
import torch

import kcore_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = ("kcore_scan", "kcore_short", "kcore_wave", "kcore_wg", "kcore_small", "kcore_publish")
INT_STATS = ("degeneracy", "rounds", "max_degree", "sub_rounds", "undirected_edges", "edges_examined", "algorithmic_bytes")


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def coo(ctx, src, dst):
    return (torch.tensor(np.asarray(src, dtype=np.int32), device=ctx.device), torch.tensor(np.asarray(dst, dtype=np.int32), device=ctx.device))


def assert_equals_reference(g, ref, what):
    """core, degree and the exact statistics of one full run against the one reference result"""
    core, degree, E, distinct = ref
    top, st = api().core_numbers(g, degree=True)
    print(what, {k: v for k, v in st.items() if not torch.is_tensor(v)})
    assert st["core"].dtype == torch.int32 and np.array_equal(st["core"].cpu().numpy(), core), what
    assert st["degree"].dtype == torch.int32 and np.array_equal(st["degree"].cpu().numpy(), degree), what
    assert top == st["degeneracy"] == (int(core.max()) if core.size else 0), what
    assert st["rounds"] == distinct, (what, st["rounds"], distinct)
    assert st["undirected_edges"] == E and st["edges_examined"] <= 2 * E, what
    assert st["max_degree"] == (int(degree.max()) if degree.size else 0), what
    assert st["algorithmic_bytes"] == 20 * g.V + 8 * st["edges_examined"], what
    return st


def launches(ctx):
    return {n: ctx.timing_get(n)[0] for n in SLOTS}


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
@pytest.mark.parametrize("renumber", [None, "total"])
def test_hand_cases(name, renumber, ctx):
    V, edges, want = R.HAND_CASES[name]
    src, dst = zip(*edges)
    ref = R.core_numbers(V, src, dst)
    assert ref[0].tolist() == want
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber=renumber)
    assert_equals_reference(g, ref, name)
    g.close()


GRAPHS = [("rmat", 10, 16, 1), ("rmat", 12, 16, 2), ("rmat", 14, 16, 3), ("rmat", 16, 16, 4), ("uniform", 12, 16, 5), ("uniform", 16, 16, 6)]


@pytest.mark.parametrize("kind,scale,ef,seed", GRAPHS)
def test_generated_graphs(kind, scale, ef, seed, ctx):
    """the directed graph, the symmetrised graph (no incoming CSR) and the renumbered graph: one reference result"""
    A = api()
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    ref = R.core_numbers(V, src.cpu().numpy(), dst.cpu().numpy())
    g = A.Graph.from_coo(ctx, V, src, dst)
    assert_equals_reference(g, ref, "directed")
    g.close()
    s = A.Graph.from_coo(ctx, V, torch.cat([src, dst]), torch.cat([dst, src]), with_incoming=False)
    assert_equals_reference(s, ref, "symmetrised")
    s.close()
    r = A.Graph.from_coo(ctx, V, src, dst, renumber="total")
    assert_equals_reference(r, ref, "renumbered")
    top, raw = A.core_numbers(r, degree=True, raw=True)                          # the graph's own numbering: original vertex bwd[i] at position i
    bwd = r.bwd.cpu().numpy()
    assert top == int(ref[0].max())
    assert np.array_equal(raw["core"].cpu().numpy(), ref[0][bwd]) and np.array_equal(raw["degree"].cpu().numpy(), ref[1][bwd])
    r.close()


def test_small_frontier_kernel_on_and_off(ctx, monkeypatch):
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 21)
    ref = R.core_numbers(V, src.cpu().numpy(), dst.cpu().numpy())
    g = A.Graph.from_coo(ctx, V, src, dst)
    g.prepare_kcore()
    seen = {}
    for small in ("0", None):
        if small is None:
            monkeypatch.delenv("VGL_KCORE_SMALL", raising=False)
        else:
            monkeypatch.setenv("VGL_KCORE_SMALL", small)
        ctx.timing(True)
        st = assert_equals_reference(g, ref, "VGL_KCORE_SMALL=%s" % small)
        seen[small] = (st, launches(ctx))
        ctx.timing(False)
    (st_off, n_off), (st_on, n_on) = seen["0"], seen[None]
    print("launches without / with the small kernel", n_off, n_on)
    assert torch.equal(st_off["core"], st_on["core"])
    assert n_off["kcore_small"] == 0 and n_on["kcore_small"] >= 1
    assert sum(n_on.values()) < sum(n_off.values())
    g.close()


SHRUNK = {"VGL_KCORE_SHORT": "2", "VGL_KCORE_WAVE": "8", "VGL_KCORE_CHUNK": "16", "VGL_KCORE_SMALL": "0", "VGL_KCORE_SORT_CAP_MB": "1"}


def test_every_class_with_shrunk_thresholds(ctx, monkeypatch):
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 11)
    ref = R.core_numbers(V, src.cpu().numpy(), dst.cpu().numpy())
    both = (torch.cat([src, dst]), torch.cat([dst, src]))
    g = A.Graph.from_coo(ctx, V, *both, with_incoming=False)
    st = assert_equals_reference(g, ref, "default thresholds")
    assert st["prepared_now"] == 1 and st["max_degree"] > 16 * 8
    for k, v in SHRUNK.items():
        monkeypatch.setenv(k, v)
    ctx.timing(True)
    st = assert_equals_reference(g, ref, "shrunk thresholds, cached symmetric CSR")
    n = launches(ctx)
    ctx.timing(False)
    print("launches under the shrunk thresholds", n)
    assert st["prepared_now"] == 0
    assert all(n[k] > 0 for k in ("kcore_scan", "kcore_short", "kcore_wave", "kcore_wg")), n
    g.close()
    # a new handle under the shrunk switches: the sort runs in pieces (262144 keys against 65536 per piece)
    g = A.Graph.from_coo(ctx, V, *both, with_incoming=False)
    st = assert_equals_reference(g, ref, "shrunk thresholds, sorted in pieces")
    assert st["prepared_now"] == 1
    monkeypatch.delenv("VGL_KCORE_SMALL")                                        # ... and the one-workgroup kernel with the shrunk classes
    assert_equals_reference(g, ref, "shrunk classes, small frontiers in one workgroup")
    g.close()


@pytest.mark.parametrize("d,want", [(4, (2, 0, 0)), (5, (1, 1, 0)), (8, (1, 1, 0)), (9, (1, 0, 1))])
def test_class_boundary_on_a_star(d, want, ctx, monkeypatch):
    """The class of a row of length d under short = 4, wave = 8 (d <= short: short, d <= wave: wave, longer: workgroup), one rule for kcore, ktruss,
    msf, msbfs and bicc.  K(1, d) on the large path: the leaves peel at k = 1 in one short launch, the hub crosses to degree 0 once and the next
    sub-round expands it in the class of its row."""
    A = api()
    for k, v in {"VGL_KCORE_SHORT": "4", "VGL_KCORE_WAVE": "8", "VGL_KCORE_SMALL": "0"}.items():
        monkeypatch.setenv(k, v)
    leaves = torch.arange(1, d + 1, dtype=torch.int32, device=ctx.device)
    g = A.Graph.from_coo(ctx, d + 1, torch.zeros_like(leaves), leaves, with_incoming=False)
    ctx.timing(True)
    top, st = A.core_numbers(g)
    n = launches(ctx)
    ctx.timing(False)
    print("K(1, %d)" % d, {k: v for k, v in st.items() if not torch.is_tensor(v)}, n)
    assert top == 1 and bool((st["core"] == 1).all())
    assert st["sub_rounds"] == 2
    assert (n["kcore_short"], n["kcore_wave"], n["kcore_wg"]) == want, n
    assert n["kcore_small"] == 0, n
    g.close()


def test_sort_cap_zero_makes_every_row_a_piece(ctx, monkeypatch):
    """VGL_KCORE_SORT_CAP_MB=0 leaves one key per piece: every row with a key exceeds it and is sorted as a piece of its own.  The 64-vertex golden
    graph, stored in both directions.  Core numbers and degrees, truss numbers with the edge endpoints (the numbering of the edges needs the rows
    sorted ACROSS the pieces) and the forest under fixed weights: equal to the references, and bit for bit what a handle built under the default
    cap returns."""
    import ktruss_reference as KT
    import msf_reference as MR
    A = api()
    raw = open(os.path.join(ROOT, "tests", "golden", "rmat_s6_e8_seed1.el_container"), "rb").read()
    V, E = int(np.frombuffer(raw, np.int32, 1, 0)[0]), int(np.frombuffer(raw, np.int64, 1, 4)[0])
    src, dst = np.frombuffer(raw, np.int32, E, 16), np.frombuffer(raw, np.int32, E, 16 + 4 * E)
    assert V == 64
    s2, d2 = np.concatenate([src, dst]), np.concatenate([dst, src])
    w = ((np.arange(2 * E, dtype=np.int64) * 7919) % 97 + 1).astype(np.float32)      # fixed; the two directions of an edge differ: the smaller counts
    core = R.core_numbers(V, s2, d2)
    eu, ev, truss, support = KT.truss_numbers(V, s2, d2)[:4]
    forest = MR.minimum_spanning_forest(V, s2, d2, w)

    def run(what):
        g = A.Graph.from_coo(ctx, V, *coo(ctx, s2, d2), with_incoming=False, want_perm=True)
        kc = assert_equals_reference(g, core, what)
        assert kc["prepared_now"] == 1
        _, kt = A.truss_numbers(g, support=True)
        total, ms = A.minimum_spanning_forest(g, ctx.gather_u32(g.perm, torch.tensor(w, device=ctx.device)), component=True, raw=True)
        g.close()
        assert np.array_equal(kt["edges"].cpu().numpy(), np.stack([eu, ev], axis=1)), what
        assert np.array_equal(kt["truss"].cpu().numpy(), truss) and np.array_equal(kt["support"].cpu().numpy(), support), what
        assert np.array_equal(ms["all_edges"].cpu().numpy(), np.stack([forest["edge_u"], forest["edge_v"]], axis=1)), what
        assert np.array_equal(ms["edge_weight"].cpu().numpy(), forest["edge_w"]) and np.array_equal(ms["in_forest"].cpu().numpy(), forest["forest"]), what
        assert np.array_equal(ms["component"].cpu().numpy(), forest["component"]) and total == forest["total"], what      # integer-valued weights: exact
        return kc, kt, ms

    default = run("default cap")
    monkeypatch.setenv("VGL_KCORE_SORT_CAP_MB", "0")
    pieces = run("one piece per row")
    for a, b in zip(default, pieces):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


def test_star_contention_on_the_hub(ctx):
    """100 000 leaves decrement one address; the hub crosses k + 1 -> k once, every later decrement is put back"""
    A = api()
    n = 100_000
    leaves = torch.arange(1, n + 1, dtype=torch.int32, device=ctx.device)
    g = A.Graph.from_coo(ctx, n + 1, torch.zeros_like(leaves), leaves, with_incoming=False)
    ctx.timing(True)
    top, st = A.core_numbers(g, degree=True)
    n_launch = launches(ctx)
    ctx.timing(False)
    print("star", {k: v for k, v in st.items() if not torch.is_tensor(v)}, n_launch)
    assert top == 1 and bool((st["core"] == 1).all()) and st["rounds"] == 1
    assert int(st["degree"][0]) == n and bool((st["degree"][1:] == 1).all())
    assert st["max_degree"] == n and st["undirected_edges"] == n and st["edges_examined"] == 2 * n
    assert n_launch["kcore_wg"] >= 1, n_launch                                   # the hub row is a workgroup-class row
    g.close()


def test_complete_bipartite_300_one_round(ctx):
    """K_{300,300}: every vertex is in the first frontier of k = 300, and every entry walked points at a vertex of that frontier"""
    A = api()
    m = 300
    a = torch.arange(m, dtype=torch.int32, device=ctx.device)
    g = A.Graph.from_coo(ctx, 2 * m, a.repeat_interleave(m), (a + m).repeat(m))
    top, st = A.core_numbers(g)
    print("K_300,300", {k: v for k, v in st.items() if not torch.is_tensor(v)})
    assert top == m and bool((st["core"] == m).all())
    assert st["rounds"] == 1 and st["sub_rounds"] == 1 and st["edges_examined"] == 2 * m * m
    g.close()


def test_clique_3000_jumps_to_its_k(ctx):
    """K_3000: k goes straight to the smallest remaining degree, 2999 -- one round, not 2999 empty shells"""
    A = api()
    n = 3000
    iu = torch.triu_indices(n, n, offset=1, device=ctx.device).to(torch.int32)
    g = A.Graph.from_coo(ctx, n, iu[0].contiguous(), iu[1].contiguous(), with_incoming=False)
    top, st = A.core_numbers(g)
    print("K_3000", {k: v for k, v in st.items() if not torch.is_tensor(v)})
    assert top == n - 1 and bool((st["core"] == n - 1).all())
    assert st["rounds"] == 1 and 1 <= st["sub_rounds"] <= 9
    g.close()


@pytest.mark.parametrize("small", ["0", None])
def test_long_tail_path_on_a_clique(small, ctx, monkeypatch):
    """a path of 4096 vertices hanging off one vertex of K_8: the peel from the free end is 4096 sub-rounds of one vertex each"""
    A = api()
    if small is not None:
        monkeypatch.setenv("VGL_KCORE_SMALL", small)
    n = 4096
    edges = R._clique(8) + [(7, 8)] + [(i, i + 1) for i in range(8, 8 + n - 1)]
    src, dst = zip(*edges)
    g = A.Graph.from_coo(ctx, 8 + n, *coo(ctx, src, dst))
    ctx.timing(True)
    top, st = A.core_numbers(g)
    n_launch = launches(ctx)
    ctx.timing(False)
    print("path on K_8, VGL_KCORE_SMALL=%s" % small, {k: v for k, v in st.items() if not torch.is_tensor(v)}, n_launch)
    core = st["core"].cpu().numpy()
    assert top == 7 and core[:8].tolist() == [7] * 8 and bool((core[8:] == 1).all())
    assert st["rounds"] == 2 and st["sub_rounds"] == n + 1
    if small is None:
        assert n_launch["kcore_small"] >= 1 and sum(n_launch.values()) <= 8, n_launch
    else:
        assert n_launch["kcore_small"] == 0
    g.close()


def test_k_limit_and_k_core(ctx):
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 31)
    core, degree, E, distinct = R.core_numbers(V, src.cpu().numpy(), dst.cpu().numpy())
    top = int(core.max())
    g = A.Graph.from_coo(ctx, V, src, dst, renumber="total")
    for k_limit in (1, 3, top, top + 5):
        want = R.core_numbers(V, src.cpu().numpy(), dst.cpu().numpy(), k_limit)
        got, st = A.core_numbers(g, k_limit=k_limit)
        assert np.array_equal(st["core"].cpu().numpy(), np.minimum(core, k_limit)) and np.array_equal(want[0], np.minimum(core, k_limit)), k_limit
        assert got == st["degeneracy"] == min(top, k_limit) and st["rounds"] == want[3], (k_limit, st["rounds"], want[3])
        member = A.k_core(g, k_limit)
        assert member.dtype == torch.bool and np.array_equal(member.cpu().numpy(), core >= k_limit), k_limit
    g.close()


def test_two_runs_agree_and_prepare_is_cached(ctx):
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 13)
    ref = R.core_numbers(V, src.cpu().numpy(), dst.cpu().numpy())
    g = A.Graph.from_coo(ctx, V, src, dst)
    _, s0 = A.core_numbers(g, degree=True)
    _, s1 = A.core_numbers(g, degree=True)
    assert s0["prepared_now"] == 1 and s1["prepared_now"] == 0
    assert torch.equal(s0["core"], s1["core"]) and torch.equal(s0["degree"], s1["degree"])
    assert all(s0[k] == s1[k] for k in INT_STATS), (s0, s1)
    assert np.array_equal(s0["core"].cpu().numpy(), ref[0])
    g.close()
    p = A.Graph.from_coo(ctx, V, src, dst)
    p.prepare_kcore()
    _, s2 = A.core_numbers(p)
    assert s2["prepared_now"] == 0 and torch.equal(s2["core"], s0["core"])
    p.close()


def test_errors(ctx):
    A = api()
    V = 1 << 10
    src, dst = ctx.gen_rmat(10, 8, 17)
    g = A.Graph.from_coo(ctx, V, src, dst)
    sh = g.shard(0, V // 2)
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        A.core_numbers(sh)
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        sh.prepare_kcore()
    with pytest.raises(A._l.VglHipError, match="d_core"):
        A._l.check(ctx.L.vgl_hip_kcore_run(ctx.h, g.h, 0, None, None, None))
    with pytest.raises(A._l.VglHipError, match="k_limit"):
        A.core_numbers(g, k_limit=-1)
    for h in (sh, g):
        h.close()


def test_kcore_app(tmp_path, ctx):
    dumps = []
    for fmt in ("csr", "vcsr"):
        dump = str(tmp_path / (fmt + ".bin"))
        cmd = [os.path.join(ROOT, "apps", "bin", "kcore_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-check", "-format", fmt, "-dump", dump]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "error count: 0" in out.stdout and "AVG_PERF" in out.stdout, out.stdout
        assert "error count" not in out.stdout.replace("error count: 0", ""), out.stdout
        dumps.append(np.fromfile(dump, np.int32))
    assert dumps[0].size == 1 << 12 and np.array_equal(dumps[0], dumps[1])
    src, dst = ctx.gen_rmat(12, 16, 1)                                           # what -gen generates: the app's default seed, the same generator
    ref = R.core_numbers(1 << 12, src.cpu().numpy(), dst.cpu().numpy())
    assert np.array_equal(dumps[0], ref[0])
