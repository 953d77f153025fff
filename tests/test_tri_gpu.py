"""Triangle counting on the GPU (vgl_hip_tri_run, api.triangle_count, apps/bin/tri_hip) against the numpy / scipy restatement of the contract
(tests/tri_reference.py) and closed forms: counts, per-vertex counts and degrees are exact, the clustering coefficient is within 1e-15 absolute of
the same float64 formula in numpy."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import tri_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def coo(ctx, src, dst):
    return (torch.tensor(np.asarray(src, dtype=np.int32), device=ctx.device), torch.tensor(np.asarray(dst, dtype=np.int32), device=ctx.device))


def assert_equals_reference(g, ref, what):
    """count alone, count + per-vertex, count + per-vertex + degree + clustering: all equal to the one reference result"""
    A = api()
    T, t, deg, E = ref
    got, st = A.triangle_count(g)
    print(what, "triangles", got, "expected", T, {k: v for k, v in st.items()})
    assert got == T and st["triangles"] == T, what
    assert st["undirected_edges"] == E and st["intersections"] == E, (what, st)
    assert "per_vertex" not in st
    got, st = A.triangle_count(g, per_vertex=True)
    assert got == T and st["per_vertex"].dtype == torch.int64 and np.array_equal(st["per_vertex"].cpu().numpy(), t), what
    got, st = A.triangle_count(g, clustering=True)
    assert got == T and np.array_equal(st["per_vertex"].cpu().numpy(), t), what
    assert st["degree"].dtype == torch.int32 and np.array_equal(st["degree"].cpu().numpy(), deg), what
    assert st["clustering"].dtype == torch.float64
    err = float(np.max(np.abs(st["clustering"].cpu().numpy() - R.clustering(t, deg)))) if t.size else 0.0
    print(what, "clustering max abs error", err)
    assert err <= 1e-15, what
    return st


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
@pytest.mark.parametrize("renumber", [None, "total"])
def test_hand_cases(name, renumber, ctx):
    V, edges, triangles, per_vertex = R.HAND_CASES[name]
    src, dst = zip(*edges)
    ref = R.triangle_count(V, src, dst)
    assert ref[0] == triangles and ref[1].tolist() == per_vertex
    g = api().Graph.from_coo(ctx, V, *coo(ctx, src, dst), renumber=renumber)
    assert_equals_reference(g, ref, name)
    g.close()


GRAPHS = [("rmat", 10, 16, 1), ("rmat", 12, 16, 2), ("rmat", 14, 16, 3), ("rmat", 16, 16, 4), ("uniform", 12, 16, 5), ("uniform", 16, 16, 6)]


@pytest.mark.parametrize("kind,scale,ef,seed", GRAPHS)
def test_generated_graphs(kind, scale, ef, seed, ctx):
    """the directed graph, the symmetrised graph (no incoming CSR: another vertex order inside) and the renumbered graph: one reference result"""
    A = api()
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    ref = R.triangle_count(V, src.cpu().numpy(), dst.cpu().numpy())
    assert int(ref[1].sum()) == 3 * ref[0]
    g = A.Graph.from_coo(ctx, V, src, dst)
    assert_equals_reference(g, ref, "directed")
    g.close()
    s = A.Graph.from_coo(ctx, V, torch.cat([src, dst]), torch.cat([dst, src]), with_incoming=False)
    assert_equals_reference(s, ref, "symmetrised")
    s.close()
    r = A.Graph.from_coo(ctx, V, src, dst, renumber="total")
    assert_equals_reference(r, ref, "renumbered")
    raw_T, raw = A.triangle_count(r, per_vertex=True, raw=True)                  # the graph's own numbering: original vertex bwd[i] at position i
    assert raw_T == ref[0] and np.array_equal(raw["per_vertex"].cpu().numpy(), ref[1][r.bwd.cpu().numpy()])
    r.close()


SHRUNK = {"VGL_TRI_LIGHT": "4", "VGL_TRI_TABLE_SMALL": "16", "VGL_TRI_TABLE": "64", "VGL_TRI_HUGE_CHUNK": "16", "VGL_TRI_SORT_CAP_MB": "1"}


def test_every_class_with_shrunk_thresholds(ctx, monkeypatch):
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 11)
    ref = R.triangle_count(V, src.cpu().numpy(), dst.cpu().numpy())
    both = (torch.cat([src, dst]), torch.cat([dst, src]))
    g = A.Graph.from_coo(ctx, V, *both, with_incoming=False)
    st = assert_equals_reference(g, ref, "default thresholds")
    assert st["rows_huge"] == 0
    for k, v in SHRUNK.items():
        monkeypatch.setenv(k, v)
    ctx.timing(True)
    st = assert_equals_reference(g, ref, "shrunk thresholds, cached oriented CSR")
    launches = {n: ctx.timing_get(n)[0] for n in ("tri_light", "tri_table", "tri_huge")}
    ctx.timing(False)
    assert st["rows_light"] > 0 and st["rows_table"] > 0 and st["rows_huge"] > 0, st
    assert all(n > 0 for n in launches.values()), launches
    assert st["max_oriented_degree"] > 64 and st["prepared_now"] == 0
    g.close()
    # a new handle under the shrunk switches: the sort runs in pieces (131072 stored entries against 65536 keys per piece)
    g = A.Graph.from_coo(ctx, V, *both, with_incoming=False)
    T, first = A.triangle_count(g, per_vertex=True)
    assert first["prepared_now"] == 1 and T == ref[0] and np.array_equal(first["per_vertex"].cpu().numpy(), ref[1])
    assert_equals_reference(g, ref, "shrunk thresholds, sorted in pieces")
    g.close()


def test_sort_cap_zero_makes_every_row_a_piece(ctx, monkeypatch):
    """VGL_TRI_SORT_CAP_MB=0 leaves one key per piece: every row with a key exceeds it and is sorted as a piece of its own.  The 64-vertex golden
    graph, stored in both directions: equal to the reference, and bit for bit what a handle built under the default cap returns."""
    A = api()
    raw = open(os.path.join(ROOT, "tests", "golden", "rmat_s6_e8_seed1.el_container"), "rb").read()
    V, E = int(np.frombuffer(raw, np.int32, 1, 0)[0]), int(np.frombuffer(raw, np.int64, 1, 4)[0])
    src, dst = np.frombuffer(raw, np.int32, E, 16), np.frombuffer(raw, np.int32, E, 16 + 4 * E)
    assert V == 64
    both = coo(ctx, np.concatenate([src, dst]), np.concatenate([dst, src]))
    ref = R.triangle_count(V, src, dst)
    g = A.Graph.from_coo(ctx, V, *both, with_incoming=False)
    T0, st0 = A.triangle_count(g, clustering=True)
    g.close()
    monkeypatch.setenv("VGL_TRI_SORT_CAP_MB", "0")
    g = A.Graph.from_coo(ctx, V, *both, with_incoming=False)
    T1, st1 = A.triangle_count(g, clustering=True)
    assert st0["prepared_now"] == 1 and st1["prepared_now"] == 1
    assert_equals_reference(g, ref, "one piece per row")
    g.close()
    assert T1 == T0 == ref[0]
    for k in ("per_vertex", "degree", "clustering"):
        assert torch.equal(st0[k], st1[k]), k
    assert {k: v for k, v in st0.items() if not torch.is_tensor(v)} == {k: v for k, v in st1.items() if not torch.is_tensor(v)}


def test_clique_3000_exceeds_32_bits(ctx):
    """K_3000: C(3000, 3) = 4 495 501 000 > 2^32 triangles, C(2999, 2) per vertex"""
    A = api()
    n = 3000
    iu = torch.triu_indices(n, n, offset=1, device=ctx.device).to(torch.int32)
    g = A.Graph.from_coo(ctx, n, iu[0].contiguous(), iu[1].contiguous(), with_incoming=False)
    T, st = A.triangle_count(g, clustering=True)
    print("K_3000", T, {k: v for k, v in st.items() if not torch.is_tensor(v)})
    assert T == math.comb(n, 3) == 4_495_501_000 and T > 2**32
    assert bool((st["per_vertex"] == math.comb(n - 1, 2)).all()) and bool((st["degree"] == n - 1).all())
    assert bool((st["clustering"] == 1.0).all())
    assert st["undirected_edges"] == math.comb(n, 2) and st["max_oriented_degree"] == n - 1
    T2, _ = A.triangle_count(g)
    assert T2 == T
    g.close()


@pytest.mark.parametrize("huge_chunk", [None, "1024"])
def test_top_class_bipartite_plus_matching(huge_chunk, ctx, monkeypatch):
    """K_{m,m} (side A = ids 0 .. m-1, side B = m .. 2m-1) plus k disjoint extra edges inside A, m above the top class boundary (8192): k * m
    triangles, m per matched A vertex, k per B vertex, 0 elsewhere.  Under (degree, id) order the unmatched A rows have oriented degree m (the
    huge class) while the second lists hold at most 2 k entries, so the case is cheap.  The huge class of this library takes no scratch block:
    a row is ceil(d / VGL_TRI_HUGE_CHUNK) workgroup units, each with its own LDS set; the repetition shrinks the chunk, so that every huge row is
    9 units instead of 2 (the part a small scratch cap would play for a bitmap scheme)."""
    A = api()
    if huge_chunk:
        monkeypatch.setenv("VGL_TRI_HUGE_CHUNK", huge_chunk)
    m, k = 8200, 4
    a = torch.arange(m, dtype=torch.int32, device=ctx.device)
    src = torch.cat([a.repeat_interleave(m), 2 * a[:k]])
    dst = torch.cat([(a + m).repeat(m), 2 * a[:k] + 1])
    g = A.Graph.from_coo(ctx, 2 * m, src, dst)                 # with the incoming CSR: the order is by total degree
    del src, dst
    T, st = A.triangle_count(g, clustering=True)
    print("K_mm + matching", T, {k_: v for k_, v in st.items() if not torch.is_tensor(v)})
    want = np.zeros(2 * m, dtype=np.int64)
    want[:2 * k] = m
    want[m:] = k
    assert T == k * m
    assert st["rows_huge"] == m - 2 * k and st["max_oriented_degree"] == m, st
    assert np.array_equal(st["per_vertex"].cpu().numpy(), want)
    deg = np.full(2 * m, m, dtype=np.int32)
    deg[:2 * k] = m + 1
    assert np.array_equal(st["degree"].cpu().numpy(), deg)
    assert st["undirected_edges"] == m * m + k
    T2, st2 = A.triangle_count(g)
    assert T2 == T and st2["elements_examined"] == st["elements_examined"]
    g.close()


def test_determinism_cache_and_counts(ctx):
    A = api()
    V = 1 << 12
    src, dst = ctx.gen_rmat(12, 16, 13)
    ref = R.triangle_count(V, src.cpu().numpy(), dst.cpu().numpy())
    g = A.Graph.from_coo(ctx, V, src, dst)
    T0, s0 = A.triangle_count(g)
    T1, s1 = A.triangle_count(g, per_vertex=True)
    T2, s2 = A.triangle_count(g, per_vertex=True)
    assert T0 == T1 == T2 == ref[0]
    assert s0["prepared_now"] == 1 and s1["prepared_now"] == 0 and s2["prepared_now"] == 0
    assert torch.equal(s1["per_vertex"], s2["per_vertex"])
    assert s0["undirected_edges"] == ref[3]
    assert s0["elements_examined"] == s1["elements_examined"] > 0
    assert s0["algorithmic_bytes"] == 8 * V + 4 * s0["undirected_edges"] + 4 * s0["elements_examined"]
    g.close()
    p = A.Graph.from_coo(ctx, V, src, dst)
    p.prepare_triangle_count()
    T3, s3 = A.triangle_count(p)
    assert T3 == ref[0] and s3["prepared_now"] == 0
    p.close()


def test_errors(ctx):
    A = api()
    V = 1 << 10
    src, dst = ctx.gen_rmat(10, 8, 17)
    g = A.Graph.from_coo(ctx, V, src, dst)
    sh = g.shard(0, V // 2)
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        A.triangle_count(sh)
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        sh.prepare_triangle_count()
    with pytest.raises(A._l.VglHipError, match="triangles"):
        A._l.check(ctx.L.vgl_hip_tri_run(ctx.h, g.h, None, None, None, None))
    for h in (sh, g):
        h.close()


def test_tri_app(tmp_path):
    dumps = []
    for fmt in ("csr", "vcsr"):
        dump = str(tmp_path / (fmt + ".bin"))
        cmd = [os.path.join(ROOT, "apps", "bin", "tri_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-check", "-format", fmt, "-dump", dump]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "error count: 0" in out.stdout and "AVG_PERF" in out.stdout, out.stdout
        assert "error count" not in out.stdout.replace("error count: 0", ""), out.stdout
        dumps.append(np.fromfile(dump, np.int64))
    assert dumps[0].size == 1 << 12 and dumps[0].sum() > 0 and np.array_equal(dumps[0], dumps[1])
