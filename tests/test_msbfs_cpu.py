"""Multi-source BFS without a GPU: the numpy / scipy restatement of the contract (tests/msbfs_reference.py) against closed forms, an independent queue
BFS and networkx, its invariances; and the build products of the feature (header, exported symbols, Python entry points, the closeness app).
Everything is compared for equality except against networkx, which adds the harmonic terms in another order: there the bound is V * 2^-52 relative."""
import ctypes
import os
import re

import numpy as np
import pytest

import msbfs_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("reached", "dist_sum", "ecc", "harmonic")


def harmonic_sum(terms):
    """the contract's loop over (n_d, d) pairs in ascending d"""
    h = np.float64(0.0)
    for n, d in terms:
        h = h + np.float64(n) / np.float64(d)
    return float(h)


def test_path():
    n = 50
    res = R.multi_source_bfs(n, np.arange(n - 1), np.arange(1, n), range(n))
    for i in range(n):
        m = n - 1 - i
        assert res["reached"][i] == n - i and res["dist_sum"][i] == m * (m + 1) // 2 and res["ecc"][i] == m
        assert res["harmonic"][i] == harmonic_sum((1, d) for d in range(1, m + 1))
        assert np.array_equal(res["levels"][i], np.concatenate([np.full(i, -1), np.arange(1, n - i + 1)]))
    assert res["levels_total"] == n and res["max_depth"] == n - 1 and res["batches"] == 1
    assert res["edges_push"] == n * (n - 1) // 2                           # level k: the vertices k .. n - 2 have a frontier word and an entry
    back = R.multi_source_bfs(n, np.arange(n - 1), np.arange(1, n), range(n), direction="in")
    assert np.array_equal(back["reached"], np.arange(1, n + 1))


def test_star_both_ways():
    k = 30
    leaves = np.arange(1, k + 1)
    src, dst = np.concatenate([np.zeros(k, dtype=np.int64), leaves]), np.concatenate([leaves, np.zeros(k, dtype=np.int64)])
    res = R.multi_source_bfs(k + 1, src, dst, [0, 1, k])
    assert res["reached"].tolist() == [k + 1] * 3 and res["dist_sum"].tolist() == [k, 1 + 2 * (k - 1), 1 + 2 * (k - 1)]
    assert res["ecc"].tolist() == [1, 2, 2]
    assert res["harmonic"].tolist() == [float(k), harmonic_sum([(1, 1), (k - 1, 2)]), harmonic_sum([(1, 1), (k - 1, 2)])]


def test_directed_cycle():
    n = 17
    res = R.multi_source_bfs(n, np.arange(n), (np.arange(n) + 1) % n, range(n))
    assert np.all(res["reached"] == n) and np.all(res["dist_sum"] == n * (n - 1) // 2) and np.all(res["ecc"] == n - 1)
    assert np.all(res["harmonic"] == harmonic_sum((1, d) for d in range(1, n)))
    assert res["levels_total"] == n and res["edges_push"] == n * n          # n levels, every vertex in every frontier


def test_complete_bipartite():
    m = 12
    a, b = np.repeat(np.arange(m), m), np.tile(np.arange(m, 2 * m), m)
    res = R.multi_source_bfs(2 * m, np.concatenate([a, b]), np.concatenate([b, a]), range(2 * m))
    assert np.all(res["reached"] == 2 * m) and np.all(res["dist_sum"] == m + 2 * (m - 1)) and np.all(res["ecc"] == 2)
    assert np.all(res["harmonic"] == harmonic_sum([(m, 1), (m - 1, 2)]))


def test_two_components_and_an_isolated_source():
    # a triangle stored one way round, a two-cycle, vertex 5 alone
    src, dst = np.array([0, 1, 2, 3, 4]), np.array([1, 2, 0, 4, 3])
    res = R.multi_source_bfs(6, src, dst, [0, 3, 5, 5])
    assert res["reached"].tolist() == [3, 2, 1, 1] and res["dist_sum"].tolist() == [3, 1, 0, 0] and res["ecc"].tolist() == [2, 1, 0, 0]
    assert res["harmonic"].tolist() == [1.5, 1.0, 0.0, 0.0]
    assert res["levels"][2].tolist() == [-1, -1, -1, -1, -1, 1]
    assert res["levels_total"] == 3 and res["reached_total"] == 7
    assert R.closeness(res, 6, wf_improved=False).tolist() == [2.0 / 3.0, 1.0, 0.0, 0.0]


def random_multigraph(rng, V, E):
    """seeded stored entries with multi-edges and loops"""
    src, dst = rng.integers(0, V, E), rng.integers(0, V, E)
    dup = rng.integers(0, max(E, 1), E // 4)
    loops = rng.integers(0, V, 5)
    return np.concatenate([src, src[dup], loops]), np.concatenate([dst, dst[dup], loops])


@pytest.mark.parametrize("V,E,seed", [(40, 120, 1), (150, 400, 2), (200, 2000, 3), (17, 0, 4), (130, 140, 5)])
@pytest.mark.parametrize("direction", ["out", "in"])
def test_restatement_equals_queue_bfs(V, E, seed, direction):
    src, dst = random_multigraph(np.random.default_rng(seed), V, E)
    sources = list(range(V)) + [0, 0]                                      # more than two batches, duplicates across batches
    res = R.multi_source_bfs(V, src, dst, sources, direction)
    for j, s in enumerate(sources):
        dist = R.queue_bfs(V, src, dst, s, direction)
        assert np.array_equal(res["levels"][j], np.where(dist >= 0, dist + 1, -1)), (j, s)
        assert (int(res["reached"][j]), int(res["dist_sum"][j]), int(res["ecc"][j]), float(res["harmonic"][j])) == R.sums_of(dist), (j, s)
    assert res["batches"] == -(-len(sources) // 64) and res["reached_total"] == int(res["reached"].sum())


def test_restatement_equals_networkx():
    nx = pytest.importorskip("networkx")
    V = 300
    rng = np.random.default_rng(7)
    src, dst = rng.integers(0, V, 1500), rng.integers(0, V, 1500)
    G = nx.DiGraph()
    G.add_nodes_from(range(V))
    G.add_edges_from(zip(src.tolist(), dst.tolist()))
    res = R.multi_source_bfs(V, src, dst, range(V), "in", want_levels=False)
    bound = V * 2.0 ** -52
    for wf in (True, False):
        want = nx.closeness_centrality(G, wf_improved=wf)
        got = R.closeness(res, V, wf)
        err = max(abs(got[v] - want[v]) / max(want[v], 1e-300) for v in range(V) if want[v] > 0)
        print("closeness wf_improved", wf, "largest relative error", err, "bound", bound)
        assert err <= bound and all(got[v] == 0 for v in range(V) if want[v] == 0)
    want = nx.harmonic_centrality(G)
    err = max(abs(res["harmonic"][v] - want[v]) / max(want[v], 1e-300) for v in range(V) if want[v] > 0)
    print("harmonic largest relative error", err, "bound", bound)
    assert err <= bound
    ecc = R.multi_source_bfs(V, src, dst, range(V), "out", want_levels=False)["ecc"]
    for v in range(0, V, 17):
        assert ecc[v] == max(nx.single_source_shortest_path_length(G, v).values())


def test_invariant_under_relabelling_and_entry_order():
    rng = np.random.default_rng(9)
    V = 150
    src, dst = random_multigraph(rng, V, 900)
    sources = rng.integers(0, V, 70)
    res = R.multi_source_bfs(V, src, dst, sources)
    perm = rng.permutation(V)                                              # vertex v becomes perm[v]
    res2 = R.multi_source_bfs(V, perm[src], perm[dst], perm[sources])
    for k in KEYS + ("levels_total", "reached_total", "edges_push", "max_depth"):
        assert np.array_equal(res2[k], res[k]), k
    assert np.array_equal(res2["levels"][:, perm], res["levels"])
    order = rng.permutation(src.size)
    res3 = R.multi_source_bfs(V, src[order], dst[order], sources)
    for k in KEYS + ("levels", "levels_total", "reached_total", "edges_push"):
        assert np.array_equal(res3[k], res[k]), k


def test_deep_path_takes_about_a_second():
    n = 5000
    res = R.multi_source_bfs(n, np.arange(n - 1), np.arange(1, n), [0, 2500, 4999, 0], want_levels=False)
    assert res["reached"].tolist() == [n, n - 2500, 1, n] and res["ecc"].tolist() == [n - 1, n - 2501, 0, n - 1]
    assert res["levels_total"] == n
    # vertex k carries sources 0 and 3 at level k (4999 vertices with an entry), vertex 2500 + k source 1 (2499 with an entry); they never meet
    assert res["edges_push"] == 4999 + 2499


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


def test_header_declares_msbfs(built):
    text = open(os.path.join(ROOT, "include", "vgl_hip.h")).read()
    assert re.search(r"\bint vgl_hip_msbfs_run\s*\(", text) and re.search(r"\bint vgl_hip_msbfs_prepare\s*\(", text)
    assert re.search(r"\}\s*vgl_hip_msbfs_stats\s*;", text)


def test_library_exports_msbfs(built):
    from vectorgraphlibrary_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "vgl_hip_msbfs_run") and hasattr(L, "vgl_hip_msbfs_prepare")
    assert "vgl_hip_msbfs_run" in lib.EXPORTED_SYMBOLS and "vgl_hip_msbfs_prepare" in lib.EXPORTED_SYMBOLS
    text = open(os.path.join(ROOT, "include", "vgl_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*vgl_hip_msbfs_stats\s*;", text).group(1)
    fields = re.findall(r"\bint(?:32|64)_t\s+([a-z_0-9]+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [f for f, _ in lib.MsbfsStats._fields_] == fields == ["sources", "batches", "max_depth", "prepared_now", "levels_push", "levels_pull",
                                                                 "levels_total", "reached_total", "edges_push", "edges_pull", "algorithmic_bytes"]
    widths = {n: w for w, n in re.findall(r"\bint(32|64)_t\s+([a-z_0-9]+)\s*;", body)}
    for name, ctype in lib.MsbfsStats._fields_:
        assert ctypes.sizeof(ctype) * 8 == int(widths[name]), name


def test_python_entry_points(built):
    from vectorgraphlibrary_amd import api
    for f in (api.multi_source_bfs, api.closeness_centrality, api.harmonic_centrality, api.eccentricity, api.Graph.prepare_msbfs):
        assert callable(f)


def test_closeness_app_built(built):
    assert os.access(os.path.join(ROOT, "apps", "bin", "closeness_hip"), os.X_OK)
