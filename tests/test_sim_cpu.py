"""The restatement of the vertex similarity contract (tests/sim_reference.py) against a brute force over Python sets and against closed forms.
No GPU: what the GPU tests compare the HIP path with is checked here first."""
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import sim_reference as R


def all_pairs(V):
    return [(a, b) for a in range(V) for b in range(V)]


def check_against_brute_force(V, stored, G, label=None):
    N = R.brute_sets(V, stored)
    pairs = all_pairs(V)
    u, v = np.asarray([a for a, _ in pairs], dtype=np.int64), np.asarray([b for _, b in pairs], dtype=np.int64)
    assert R.common(G, u, v).tolist() == R.brute_common(N, pairs)
    edges = sorted((a, b) for a in range(V) for b in N[a] if a < b)
    for block in (1, 3, 1024):
        eu, ev, ec = R.edge_common(G, block)
        assert list(zip(eu.tolist(), ev.tolist())) == edges and ec.tolist() == R.brute_common(N, edges)
    assert G["deg"].tolist() == [len(s) for s in N]
    assert G["work2"].tolist() == [sum(len(N[w]) for w in N[a]) for a in range(V)]
    for metric, include, k in itertools.product(R.METRICS, (False, True), (1, 3, 64)):
        ref = R.topk(G, None, k, metric, include, label)
        for a in range(V):
            want = R.brute_topk(N, a, k, metric, include, label)
            got = [(int(w), int(c)) for w, c in zip(ref["ids"][a], ref["common"][a]) if w >= 0]
            assert got == want, (metric, include, k, a)
            assert all(w == -1 and c == 0 for w, c in zip(ref["ids"][a][len(want):], ref["common"][a][len(want):]))
        assert ref["filled"] == int((ref["ids"] >= 0).sum())
        assert ref["candidates_total"] == sum(len(R.brute_topk(N, a, V, metric, include, label)) for a in range(V))
        assert ref["two_paths_walked"] == int(G["work2"].sum())


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_hand_cases_against_brute_force(name):
    V, src, dst, G = R.hand_graph(name)
    check_against_brute_force(V, R.HAND_CASES[name][1], G)
    check_against_brute_force(V, R.HAND_CASES[name][1], G, label=np.arange(V)[::-1].copy())


def test_complete_graph():
    V, src, dst, G = R.hand_graph("k6")
    a, b = np.triu_indices(6, 1)
    assert (R.common(G, a, b) == 4).all() and (R.common(G, np.arange(6), np.arange(6)) == 5).all()      # n - 2; u == v: d(u)
    ref = R.topk(G, None, 3, R.JACCARD)
    assert (ref["ids"] == -1).all() and ref["candidates_total"] == 0 and ref["filled"] == 0               # every 2-hop vertex is a neighbour
    ref = R.topk(G, None, 3, R.JACCARD, include_neighbours=True)
    assert ref["ids"][0].tolist() == [1, 2, 3] and ref["ids"][5].tolist() == [0, 1, 2] and (ref["common"] == 4).all()


def test_complete_bipartite_3_4():
    V, src, dst, G = R.hand_graph("k34")
    assert R.common(G, [0, 0, 1], [1, 2, 2]).tolist() == [4, 4, 4]                  # the side of 3: the 4 others
    assert R.common(G, [3, 3, 5], [4, 6, 6]).tolist() == [3, 3, 3]                  # the side of 4: the 3 others
    assert R.common(G, [0, 2], [3, 6]).tolist() == [0, 0]                           # across: adjacent, nothing in common
    assert R.score(R.JACCARD, [4, 3], [4, 3], [4, 3]).tolist() == [1.0, 1.0]
    ref = R.topk(G, None, 5, R.JACCARD)
    assert ref["ids"][0].tolist() == [1, 2, -1, -1, -1] and ref["ids"][2].tolist() == [0, 1, -1, -1, -1]      # ties by id
    assert ref["ids"][4].tolist() == [3, 5, 6, -1, -1] and ref["common"][4].tolist() == [3, 3, 3, 0, 0]
    rev = R.topk(G, None, 5, R.JACCARD, label=np.arange(7)[::-1].copy())
    assert rev["ids"][4].tolist() == [6, 5, 3, -1, -1]                               # ... by label when one is given


def test_path_5():
    V, src, dst, G = R.hand_graph("path5")
    assert R.common(G, [0, 1, 0, 0, 2], [2, 3, 1, 3, 2]).tolist() == [1, 1, 0, 0, 2]     # distance 2; adjacent; distance 3; u == v
    ref = R.topk(G, None, 2, R.JACCARD)
    assert ref["ids"].tolist() == [[2, -1], [3, -1], [0, 4], [1, -1], [2, -1]]           # 2: J(2, 0) = J(2, 4) = 1 / 2, the smaller id first
    assert ref["candidates_total"] == 6 and ref["filled"] == 6
    ref = R.topk(G, [1], 2, R.OVERLAP)
    assert ref["ids"].tolist() == [[3, -1]] and ref["common"].tolist() == [[1, 0]]


def test_star():
    V, src, dst, G = R.hand_graph("star")
    a, b = np.triu_indices(6, 1)
    assert (R.common(G, a + 1, b + 1) == 1).all()
    assert (R.score(R.JACCARD, 1, 1, 1) == 1.0).all()
    ref = R.topk(G, [3, 0, 7], 64, R.COMMON)
    assert ref["ids"][0][:6].tolist() == [1, 2, 4, 5, 6, -1] and (ref["ids"][1:] == -1).all()        # the hub's 2-hop vertices are itself; 7 is isolated
    assert ref["two_paths_walked"] == 6 + 6 + 0


def test_two_triangles_sharing_a_vertex():
    V, src, dst, G = R.hand_graph("two_triangles_sharing_a_vertex")
    assert R.common(G, [0, 0, 0, 3], [1, 2, 3, 4]).tolist() == [1, 1, 1, 1]
    ref = R.topk(G, [0], 4, R.JACCARD)
    assert ref["ids"].tolist() == [[3, 4, -1, -1]] and ref["common"].tolist() == [[1, 1, 0, 0]]
    ref = R.topk(G, [0], 4, R.JACCARD, include_neighbours=True)
    assert ref["ids"].tolist() == [[1, 3, 4, 2]]            # 1 / 3 (N(0) | N(1) = {0, 1, 2}), 1 / 3, 1 / 3, then 2: 1 / 5


def test_edgeless_graph():
    V, src, dst, G = R.hand_graph("edgeless")
    assert R.common(G, [0, 1, 2], [1, 1, 3]).tolist() == [0, 0, 0]
    ref = R.topk(G, None, 2, R.COMMON, include_neighbours=True)
    assert (ref["ids"] == -1).all() and ref["candidates_total"] == 0 and ref["two_paths_walked"] == 0
    assert R.score(R.JACCARD, [0], [0], [0]).tolist() == [0.0] and R.score(R.OVERLAP, [0], [0], [0]).tolist() == [0.0]


def test_loops_and_duplicates_do_not_count():
    V, src, dst, G = R.hand_graph("loops_and_duplicates")
    plain = R.simple_graph(5, [0, 1, 0, 2, 3], [1, 2, 2, 3, 4])
    assert (G["A"] != plain["A"]).nnz == 0 and G["deg"].tolist() == [2, 2, 3, 2, 1]
    assert R.common(G, [0, 0, 1, 2], [1, 3, 3, 2]).tolist() == [1, 1, 1, 3]


def test_sorensen_ranks_exactly_as_jaccard():
    rng = np.random.default_rng(7)
    V = 200
    src, dst = rng.integers(0, V, 1500), rng.integers(0, V, 1500)
    G = R.simple_graph(V, src, dst)
    check_against_brute_force(V, list(zip(src.tolist(), dst.tolist())), G)
    for u in range(V):
        for include in (False, True):
            j = R.ranked(G, u, R.JACCARD, include)
            s = R.ranked(G, u, "sorensen", include)
            assert np.array_equal(j[0], s[0]) and np.array_equal(j[1], s[1])
            num, den = R.fraction(R.JACCARD, j[1], G["deg"][u], G["deg"][j[0]])
            J = [Fraction(int(a), int(b)) for a, b in zip(num, den)]
            assert all(x >= y for x, y in zip(J, J[1:]))                       # best first
            assert [2 * x / (1 + x) for x in J] == [Fraction(2 * int(c), int(G["deg"][u] + G["deg"][w])) for w, c in zip(*j)]


def test_the_prefilter_of_ranked_keeps_the_order():
    rng = np.random.default_rng(11)
    V = 300
    src, dst = rng.integers(0, V, 4000), rng.integers(0, V, 4000)
    G = R.simple_graph(V, src, dst)
    for u in range(0, V, 7):
        for metric in R.METRICS:
            full = R.ranked(G, u, metric)
            for k in (1, 10, 64):
                part = R.ranked(G, u, metric, k=k)
                assert np.array_equal(part[0], full[0][:k]) and np.array_equal(part[1], full[1][:k])


def test_weighted_sums_and_statistics():
    V, src, dst, G = R.hand_graph("two_triangles_sharing_a_vertex")
    aa, hits = R.weighted(G, [0, 0, 2], [1, 3, 2], R.adamic_adar_weights(G["deg"]))
    assert hits.tolist() == [1, 1, 4]
    assert aa.tolist() == [1.0 / math.log(4.0), 1.0 / math.log(4.0), math.fsum([1.0 / math.log(2.0)] * 4)]
    ra, _ = R.weighted(G, [0, 0, 2], [1, 3, 2], R.resource_allocation_weights(G["deg"]))
    assert ra.tolist() == [0.25, 0.25, 2.0]
    st = R.pair_stats(G, [0, 0, 2], [1, 3, 2], short=2, wave=3)
    assert st == {"pairs": 3, "pairs_short": 2, "pairs_wave": 0, "pairs_wg": 1, "elements_examined": 2 + 2 + 4, "common_total": 1 + 1 + 4}
    assert R.topk_rows(G, None, small=4, table=6) == {"rows_small": 0, "rows_table": 4, "rows_global": 1}        # work2 = 6, 6, 8, 6, 6


def test_the_scores_of_the_python_layer_match_the_restatement():
    import torch
    from vectorgraphlibrary_amd import api
    rng = np.random.default_rng(3)
    du, dv = rng.integers(0, 50, 1000), rng.integers(0, 50, 1000)
    c = rng.integers(0, np.minimum(du, dv) + 1)
    for metric in ("common", "jaccard", "overlap", "sorensen"):
        got = api._sim_score(metric, torch.tensor(c), torch.tensor(du), torch.tensor(dv)).numpy()
        np.testing.assert_allclose(got, R.score(metric, c, du, dv), rtol=4e-16, atol=0.0)
    assert api._SIM_CODES["sorensen"] == api._SIM_CODES["jaccard"] == api.SIM_JACCARD


def test_built_library_exports_the_entry_points():
    import ctypes
    import os
    import __graft_entry__ as ge
    ge.build()
    from vectorgraphlibrary_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    for s in ("vgl_hip_sim_prepare", "vgl_hip_sim_pairs", "vgl_hip_sim_topk"):
        assert hasattr(L, s), s
    assert os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "apps", "bin", "sim_hip"))
    assert ctypes.sizeof(lib.SimPairsStats) == 64 and ctypes.sizeof(lib.SimTopkStats) == 80
