"""Triangle counting without a GPU: the numpy / scipy restatement of the contract (tests/tri_reference.py) on hand-checked cases and against dense
A^3, and the build products of the feature (header, exported symbols, Python entry points, the tri app)."""
import ctypes
import os
import re

import numpy as np
import pytest

import tri_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_restatement_hand_cases(name):
    V, edges, triangles, per_vertex = R.HAND_CASES[name]
    src, dst = zip(*edges)
    T, t, deg, E = R.triangle_count(V, src, dst)
    assert t.dtype == np.int64 and deg.dtype == np.int32
    assert T == triangles and t.tolist() == per_vertex
    assert int(t.sum()) == 3 * T
    assert E == len({(min(a, b), max(a, b)) for a, b in edges if a != b}) and int(deg.sum()) == 2 * E


def random_multigraph(rng, V, E):
    """seeded stored entries with multi-edges, loops and both directions"""
    src = rng.integers(0, V, E)
    dst = rng.integers(0, V, E)
    dup = rng.integers(0, E, E // 4)
    loops = rng.integers(0, V, 5)
    return np.concatenate([src, src[dup], dst[dup[:10]], loops]), np.concatenate([dst, dst[dup], src[dup[:10]], loops])


@pytest.mark.parametrize("V,E,seed", [(40, 200, 1), (120, 2000, 2), (200, 1500, 3), (200, 12000, 4), (17, 0, 5)])
def test_restatement_equals_dense_cube(V, E, seed):
    src, dst = random_multigraph(np.random.default_rng(seed), V, E)
    T, t, deg, _ = R.triangle_count(V, src, dst)
    bT, bt, bdeg = R.brute_force(V, src, dst)
    assert T == bT and np.array_equal(t, bt) and np.array_equal(deg, bdeg)
    assert int(t.sum()) == 3 * T


def test_restatement_invariant_under_relabelling_and_order():
    rng = np.random.default_rng(9)
    V = 150
    src, dst = random_multigraph(rng, V, 3000)
    T, t, deg, E = R.triangle_count(V, src, dst)
    perm = rng.permutation(V)                                     # vertex v becomes perm[v]
    T2, t2, deg2, E2 = R.triangle_count(V, perm[src], perm[dst])
    assert T2 == T and E2 == E and np.array_equal(t2[perm], t) and np.array_equal(deg2[perm], deg)
    T3, t3, _, _ = R.triangle_count(V, src, dst, rank=rng.permutation(V))       # any total order
    assert T3 == T and np.array_equal(t3, t)


def test_clustering_formula():
    V, edges, _, _ = R.HAND_CASES["two_triangles_sharing_an_edge"]
    src, dst = zip(*edges)
    _, t, deg, _ = R.triangle_count(V, src, dst)
    assert R.clustering(t, deg).tolist() == [1.0, 2.0 / 3.0, 2.0 / 3.0, 1.0]
    assert R.clustering(np.array([0, 0]), np.array([0, 1])).tolist() == [0.0, 0.0]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_header_declares_tri(built):
    text = open(os.path.join(ROOT, "include", "vgl_hip.h")).read()
    assert re.search(r"\bint vgl_hip_tri_run\s*\(", text) and re.search(r"\bint vgl_hip_tri_prepare\s*\(", text)
    assert "vgl_hip_tri_stats" in text


def test_library_exports_tri(built):
    from vectorgraphlibrary_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "vgl_hip_tri_run") and hasattr(L, "vgl_hip_tri_prepare")
    assert "vgl_hip_tri_run" in lib.EXPORTED_SYMBOLS and "vgl_hip_tri_prepare" in lib.EXPORTED_SYMBOLS
    assert [f for f, _ in lib.TriStats._fields_] == ["triangles", "undirected_edges", "intersections", "elements_examined", "algorithmic_bytes",
                                                      "max_oriented_degree", "prepared_now", "rows_light", "rows_table", "rows_huge"]


def test_python_entry_points(built):
    from vectorgraphlibrary_amd import api
    assert callable(api.triangle_count) and callable(api.Graph.prepare_triangle_count)


def test_tri_app_built(built):
    assert os.access(os.path.join(ROOT, "apps", "bin", "tri_hip"), os.X_OK)
