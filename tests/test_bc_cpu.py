"""Betweenness centrality without a GPU: the numpy / scipy restatement of the contract (tests/bc_reference.py) on hand cases with closed forms, against
an independent brute force and networkx, its invariances and the certificate; and the build products of the feature (header, exported symbols, Python
entry points, the bc app).  The tolerance is bc_reference.tolerance (derived in DESIGN section 14), from each case's own D, d_max and S."""
import ctypes
import os
import re

import numpy as np
import pytest

import bc_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_within(got, ref, info, what):
    tol = R.tolerance(info["max_depth"], info["d_max"], info["sources"])
    ok, frac = R.compare(got, ref, tol)
    print(what, "largest error / bound", frac, "bound", tol)
    assert ok, (what, frac)


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_restatement_hand_cases(name):
    V, edges, want = R.HAND_CASES[name]
    src, dst = zip(*edges)
    bc, info = R.betweenness(V, src, dst)
    assert bc.dtype == np.float64 and info["sources"] == V
    assert_within(bc, np.array(want), info, name)
    assert info["sigma_max"] < 2.0 ** 53


def random_multigraph(rng, V, E):
    """seeded stored entries with multi-edges, loops and some edges in both directions"""
    src = rng.integers(0, V, E)
    dst = rng.integers(0, V, E)
    dup = rng.integers(0, max(E, 1), E // 4)
    loops = rng.integers(0, V, 5)
    return np.concatenate([src, src[dup], dst[dup[:10]], loops]), np.concatenate([dst, dst[dup], src[dup[:10]], loops])


@pytest.mark.parametrize("V,E,seed", [(40, 120, 1), (120, 500, 2), (200, 900, 3), (200, 4000, 4), (17, 0, 5), (60, 70, 6)])
def test_restatement_equals_brute_force(V, E, seed):
    src, dst = random_multigraph(np.random.default_rng(seed), V, E)
    bc, info = R.betweenness(V, src, dst)
    assert_within(bc, R.brute_force(V, src, dst), info, "brute force")


@pytest.mark.parametrize("V,E,seed", [(120, 500, 2), (200, 4000, 4)])
def test_restatement_equals_networkx(V, E, seed):
    nx = pytest.importorskip("networkx")
    src, dst = random_multigraph(np.random.default_rng(seed), V, E)
    pairs = sorted(set(zip(src.tolist(), dst.tolist())))                   # networkx ignores multiplicities
    G = nx.DiGraph()
    G.add_nodes_from(range(V))
    G.add_edges_from(pairs)
    want = nx.betweenness_centrality(G, normalized=False)
    s, d = zip(*pairs)
    bc, info = R.betweenness(V, s, d)
    assert_within(bc, np.array([want[v] for v in range(V)]), info, "networkx")


def test_restatement_invariant_under_relabelling_and_entry_order():
    rng = np.random.default_rng(9)
    V = 150
    src, dst = random_multigraph(rng, V, 1200)
    bc, info = R.betweenness(V, src, dst)
    perm = rng.permutation(V)                                              # vertex v becomes perm[v]
    bc2, info2 = R.betweenness(V, perm[src], perm[dst])
    assert_within(bc2[perm], bc, info, "relabelled")
    for k in ("max_depth", "levels_total", "reached_total", "edges_forward", "edges_backward"):
        assert info2[k] == info[k], k
    order = rng.permutation(src.size)                                      # the entries of every row in another order
    bc3, _ = R.betweenness(V, src[order], dst[order])
    assert_within(bc3, bc, info, "entries permuted")


def test_restatement_sampled_sources_add_up():
    rng = np.random.default_rng(11)
    V = 100
    src, dst = random_multigraph(rng, V, 600)
    a, b = list(range(0, 40)), list(range(40, V))
    bc_a, _ = R.betweenness(V, src, dst, a)
    bc_b, _ = R.betweenness(V, src, dst, b)
    bc, info = R.betweenness(V, src, dst)
    assert_within(bc_a + bc_b, bc, info, "A + B")


@pytest.mark.parametrize("V,E,seed", [(120, 500, 2), (200, 4000, 4), (60, 70, 6)])
def test_certificate_on_the_restatement(V, E, seed):
    src, dst = random_multigraph(np.random.default_rng(seed), V, E)
    A, AT = R.count_matrix(V, src, dst)
    d_max = int(max(A.sum(axis=1).max(), AT.sum(axis=1).max()))
    for s in range(0, V, 7):
        levels, sigma, delta, D = R.single_source(A, AT, s)
        want = R.certificate(levels)
        assert isinstance(want, int) and want >= 0
        tol = R.tolerance(D, d_max, 1) + V * R.U
        got = float(delta.sum() - delta[s])
        assert abs(got - want) <= tol * max(want, 1), (s, got, want)
        assert sigma[s] == 1.0 and bool(np.all((sigma > 0) == (levels > 0)))


def test_grid_sigma_is_binomial():
    n = 12
    src, dst = R.grid_both_ways(n)
    A, AT = R.count_matrix(n * n, src, dst)
    levels, sigma, _, D = R.single_source(A, AT, 0)
    assert D == 2 * (n - 1) and np.array_equal(sigma, R.grid_sigma(n))
    assert np.array_equal(levels.reshape(n, n), 1 + np.add.outer(np.arange(n), np.arange(n)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_header_declares_bc(built):
    text = open(os.path.join(ROOT, "include", "vgl_hip.h")).read()
    assert re.search(r"\bint vgl_hip_bc_run\s*\(", text) and re.search(r"\bint vgl_hip_bc_prepare\s*\(", text)
    assert re.search(r"\}\s*vgl_hip_bc_stats\s*;", text)


def test_library_exports_bc(built):
    from vectorgraphlibrary_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "vgl_hip_bc_run") and hasattr(L, "vgl_hip_bc_prepare")
    assert "vgl_hip_bc_run" in lib.EXPORTED_SYMBOLS and "vgl_hip_bc_prepare" in lib.EXPORTED_SYMBOLS
    text = open(os.path.join(ROOT, "include", "vgl_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*vgl_hip_bc_stats\s*;", text).group(1)
    fields = re.findall(r"\bint(?:32|64)_t\s+([a-z_0-9]+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [f for f, _ in lib.BcStats._fields_] == fields == ["sources", "max_depth", "sigma_inexact", "prepared_now", "levels_total", "reached_total",
                                                              "edges_forward", "edges_backward", "algorithmic_bytes"]
    widths = {n: w for w, n in re.findall(r"\bint(32|64)_t\s+([a-z_0-9]+)\s*;", body)}
    for name, ctype in lib.BcStats._fields_:
        assert ctypes.sizeof(ctype) * 8 == int(widths[name]), name


def test_python_entry_points(built):
    from vectorgraphlibrary_amd import api
    assert callable(api.betweenness_centrality) and callable(api.Graph.prepare_betweenness)


def test_bc_app_built(built):
    assert os.access(os.path.join(ROOT, "apps", "bin", "bc_hip"), os.X_OK)
