"""CPU tests of the minimum spanning forest contract: the numpy restatement (tests/msf_reference.py) on hand-made cases, against
networkx.minimum_spanning_edges, scipy's minimum_spanning_tree and connected_components, and the C ABI (include/vgl_hip.h declares the two entry
points, the built library exports them, the ctypes struct has the header's layout)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components, minimum_spanning_tree

import msf_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_restatement_equals_hand_cases(name):
    V, src, dst, w, want = R.hand_case(name)
    m = R.minimum_spanning_forest(V, src, dst, w)
    got = sorted(zip(m["edge_u"][m["forest"]].tolist(), m["edge_v"][m["forest"]].tolist()))
    assert got == want, name
    assert m["edge_u"].dtype == m["edge_v"].dtype == m["component"].dtype == np.int32 and m["edge_w"].dtype == np.float32
    assert m["forest_edges"] == len(want) and m["components"] == V - len(want)
    assert (m["rounds"] == 0) == (m["undirected_edges"] == 0) and m["rounds"] <= max(0, math.ceil(math.log2(V)))
    assert np.array_equal(m["component"][m["component"]], m["component"]) and bool((m["component"] <= np.arange(V)).all())
    assert not np.signbit(m["edge_w"][m["edge_w"] == 0]).any()                  # -0.0 is folded to +0.0


def test_fold_takes_the_lightest_copy_in_either_direction():
    V, src, dst, w, _ = R.hand_case("ring_5_both_ways_and_duplicates")
    eu, ev, ew = R.folded(V, src, dst, w)
    assert list(zip(eu.tolist(), ev.tolist(), ew.tolist())) == [(0, 1, 1.0), (0, 4, 5.0), (1, 2, 2.0), (2, 3, 3.0), (3, 4, 4.0)]


def test_nan_is_refused_unless_on_a_loop():
    with pytest.raises(ValueError, match="weights"):
        R.folded(3, [0, 1], [1, 2], [1.0, float("nan")])
    eu, ev, ew = R.folded(3, [0, 1, 1], [1, 2, 1], [1.0, 2.0, float("nan")])
    assert ew.tolist() == [1.0, 2.0]


def test_ruler_takes_a_round_per_level_and_star_takes_one():
    V, src, dst, w = R.ruler(256, 20)
    m = R.minimum_spanning_forest(V, src, dst, w)
    assert m["rounds"] >= 7 and m["forest_edges"] == V - 1
    V, src, dst, w = R.star(50)
    m = R.minimum_spanning_forest(V, src, dst, w)
    assert m["rounds"] == 1 and m["forest_edges"] == 50 and bool(m["forest"].all())


def _random_graph(rng, V, E, skew):
    if skew:                                     # a few heavy vertices: a dense core over a sparse fringe
        p = 1.0 / np.arange(1, V + 1) ** 0.8
        p /= p.sum()
        src, dst = rng.choice(V, E, p=p), rng.choice(V, E, p=p)
    else:
        src, dst = rng.integers(0, V, E), rng.integers(0, V, E)
    return src.astype(np.int64), dst.astype(np.int64)


def _weights(rng, E, ties):
    """strictly positive, integer-valued: {1, 2, 3} (almost every comparison a tie) or a permutation of 1 .. E (all distinct, exact in float32)"""
    return (rng.integers(1, 4, E) if ties else rng.permutation(E) + 1).astype(np.float32)


CASES = [(300, 3000, False, 1, False), (800, 12000, True, 2, False), (2000, 30000, False, 3, False), (1500, 30000, True, 4, True)]
_RESULTS = {}


def _result(case):
    if case not in _RESULTS:
        V, E, skew, seed, ties = case
        rng = np.random.default_rng(seed)
        src, dst = _random_graph(rng, V, E, skew)                                # loops and duplicates included: the contract folds them
        _RESULTS[case] = (src, dst, R.minimum_spanning_forest(V, src, dst, _weights(rng, E, ties)))
    return _RESULTS[case]


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_networkx(case):
    import networkx as nx
    V, ties = case[0], case[4]
    _, _, m = _result(case)
    eu, ev, ew, forest = m["edge_u"], m["edge_v"], m["edge_w"], m["forest"]
    G = nx.Graph()
    G.add_nodes_from(range(V))
    G.add_weighted_edges_from(zip(eu.tolist(), ev.tolist(), ew.astype(np.float64).tolist()))
    assert G.number_of_edges() == eu.size
    tree = [(min(a, b), max(a, b)) for a, b in nx.minimum_spanning_edges(G, data=False)]
    assert len(tree) == m["forest_edges"] == V - nx.number_connected_components(G)
    if ties:                                                                   # the forest is one of several: its weight is not
        assert sum(G[a][b]["weight"] for a, b in tree) == m["total"]
    else:
        assert sorted(tree) == sorted(zip(eu[forest].tolist(), ev[forest].tolist()))
    assert 1 <= m["rounds"] <= math.ceil(math.log2(V))


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_scipy(case):
    V = case[0]
    src, dst, m = _result(case)
    eu, ev, ew = m["edge_u"], m["edge_v"], m["edge_w"]
    assert bool((ew >= 1).all()) and bool((ew == np.rint(ew)).all())             # scipy reads a zero as "no edge"
    U = sp.csr_matrix((ew.astype(np.float64), (eu, ev)), shape=(V, V))
    T = minimum_spanning_tree(U)
    assert T.nnz == m["forest_edges"] and float(T.sum()) == m["total"]
    n, lab = connected_components(sp.csr_matrix((np.ones(src.size), (src, dst)), shape=(V, V)), directed=False)
    assert n == m["components"]
    smallest = np.full(V, V, dtype=np.int64)
    np.minimum.at(smallest, lab, np.arange(V))
    assert np.array_equal(m["component"], smallest[lab])


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "vgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+vgl_hip_msf_prepare\s*\(\s*vgl_hip_ctx\s*\*\s*\w+\s*,\s*vgl_hip_graph\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+vgl_hip_msf_run\s*\([^;]*const\s+float\s*\*\s*d_weights[^;]*int32_t\s*\*\s*d_edge_u[^;]*int32_t\s*\*\s*d_edge_v[^;]*float\s*\*\s*d_edge_weight"
                     r"[^;]*uint8_t\s*\*\s*d_in_forest[^;]*int32_t\s*\*\s*d_component[^;]*vgl_hip_msf_stats\s*\*\s*\w+\s*\)\s*;", text)
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*vgl_hip_msf_stats\s*;", text)
    assert struct
    assert re.findall(r"\b(int32_t|int64_t|double)\s+(\w+)\s*;", struct.group(1)) == [
        ("int32_t", "rounds"), ("int32_t", "prepared_now"), ("int64_t", "forest_edges"), ("int64_t", "components"), ("int64_t", "undirected_edges"),
        ("int64_t", "entries_walked"), ("int64_t", "algorithmic_bytes"), ("double", "total_weight")]
    import __graft_entry__ as ge
    ge.build()
    from vectorgraphlibrary_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    for s in ("vgl_hip_msf_prepare", "vgl_hip_msf_run"):
        assert hasattr(L, s), s
        assert s in lib.EXPORTED_SYMBOLS
    fields = [(n, t, ctypes.sizeof(t)) for n, t in lib.MsfStats._fields_]
    assert fields == [("rounds", ctypes.c_int32, 4), ("prepared_now", ctypes.c_int32, 4), ("forest_edges", ctypes.c_int64, 8), ("components", ctypes.c_int64, 8),
                      ("undirected_edges", ctypes.c_int64, 8), ("entries_walked", ctypes.c_int64, 8), ("algorithmic_bytes", ctypes.c_int64, 8),
                      ("total_weight", ctypes.c_double, 8)]
    assert ctypes.sizeof(lib.MsfStats) == 56                                     # the int32 fields first, then the 64-bit fields: no padding holes
    assert lib.MsfStats.total_weight.offset == 48
    assert os.path.exists(os.path.join(ROOT, "apps", "bin", "msf_hip"))
