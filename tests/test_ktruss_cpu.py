"""CPU tests of the k-truss contract: the numpy / scipy restatement (tests/ktruss_reference.py) against closed forms and networkx.k_truss, the k_limit
rule, the triangle total against tri_reference, and the C ABI (include/vgl_hip.h declares the two entry points and the built library exports them)."""
import ctypes
import os
import re

import numpy as np
import pytest

import ktruss_reference as R
from tri_reference import triangle_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _coo(edges):
    return ([a for a, _ in edges], [b for _, b in edges])


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_restatement_equals_closed_forms(name):
    V, edges, want = R.HAND_CASES[name]
    eu, ev, truss, support, triangles, rounds, sub_rounds = R.truss_numbers(V, *_coo(edges))
    assert eu.dtype == ev.dtype == truss.dtype == support.dtype == np.int32
    assert truss.tolist() == want, name
    assert bool((eu < ev).all()) and bool((np.diff(eu.astype(np.int64) * V + ev) > 0).all())
    assert int(support.sum()) == 3 * triangles == 3 * triangle_count(V, *_coo(edges))[0]
    assert rounds == len(set(want)) and sub_rounds >= rounds
    assert bool((truss <= support + 2).all())


@pytest.mark.parametrize("make,args,truss,rounds,sub_rounds", [(R.tube, (16, True), 4, 1, 1), (R.tube, (16,), 3, 1, 32), (R.book, (50,), 3, 1, 2),
                                                                (R.tripartite, (5,), 7, 1, 1)])
def test_generators(make, args, truss, rounds, sub_rounds):
    V, src, dst = make(*args)
    got = R.truss_numbers(V, src, dst)
    assert bool((got[2] == truss).all()) and got[5:] == (rounds, sub_rounds)
    if make is R.tube and args[-1] is True:
        assert bool((got[3] == 2).all())                                         # capped at both ends: every edge in exactly two triangles
    if make is R.book:
        assert int(got[3].max()) == args[0] and got[4] == args[0]


def _random_graph(rng, V, E, skew):
    if skew:                                     # a few heavy vertices: a dense core over a sparse fringe
        p = 1.0 / np.arange(1, V + 1) ** 0.8
        p /= p.sum()
        src, dst = rng.choice(V, E, p=p), rng.choice(V, E, p=p)
    else:
        src, dst = rng.integers(0, V, E), rng.integers(0, V, E)
    return src.astype(np.int64), dst.astype(np.int64)


@pytest.mark.parametrize("V,E,skew,seed", [(300, 3000, False, 1), (800, 12000, True, 2), (2000, 30000, False, 3), (1500, 30000, True, 4)])
def test_restatement_equals_networkx(V, E, skew, seed):
    import networkx as nx
    src, dst = _random_graph(np.random.default_rng(seed), V, E, skew)          # loops and duplicates included: the contract drops them
    eu, ev, truss, support, triangles, rounds, sub_rounds = R.truss_numbers(V, src, dst)
    G = nx.Graph()                                                             # networkx refuses self-loops: it gets the simple graph
    G.add_nodes_from(range(V))
    G.add_edges_from(zip(eu.tolist(), ev.tolist()))
    assert G.number_of_edges() == eu.size
    want = {}
    k = 2
    while True:                                                                # truss(e) = the largest k with e in the k-truss
        H = nx.k_truss(G, k)
        if H.number_of_edges() == 0:
            break
        for a, b in H.edges():
            want[(min(a, b), max(a, b))] = k
        k += 1
    assert truss.tolist() == [want[e] for e in zip(eu.tolist(), ev.tolist())]
    assert int(support.sum()) == 3 * (sum(nx.triangles(G).values()) // 3) == 3 * triangles
    assert triangles == triangle_count(V, src, dst)[0]
    assert rounds == np.unique(truss).size


def test_k_limit_is_the_minimum():
    src, dst = _random_graph(np.random.default_rng(7), 1500, 30000, True)
    full = R.truss_numbers(1500, src, dst)
    top = int(full[2].max())
    assert top >= 5
    for k_limit in (2, 3, top, top + 5):
        got = R.truss_numbers(1500, src, dst, k_limit)
        assert np.array_equal(got[2], np.minimum(full[2], k_limit)) and np.array_equal(got[3], full[3]) and got[4] == full[4]
        assert got[5] == np.unique(full[2][full[2] < k_limit]).size
    for bad in (1, -1):
        with pytest.raises(ValueError):
            R.truss_numbers(1500, src, dst, bad)


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "vgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+vgl_hip_ktruss_prepare\s*\(\s*vgl_hip_ctx\s*\*\s*\w+\s*,\s*vgl_hip_graph\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+vgl_hip_ktruss_run\s*\([^;]*int32_t\s+k_limit[^;]*int32_t\s*\*\s*d_edge_u[^;]*int32_t\s*\*\s*d_edge_v[^;]*int32_t\s*\*\s*d_truss"
                     r"[^;]*int32_t\s*\*\s*d_support[^;]*vgl_hip_ktruss_stats\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\}\s*vgl_hip_ktruss_stats\s*;", text)
    import __graft_entry__ as ge
    ge.build()
    from vectorgraphlibrary_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    for s in ("vgl_hip_ktruss_prepare", "vgl_hip_ktruss_run"):
        assert hasattr(L, s), s
        assert s in lib.EXPORTED_SYMBOLS
    fields = [(n, ctypes.sizeof(t)) for n, t in lib.KtrussStats._fields_]
    assert fields == [("max_truss", 4), ("rounds", 4), ("max_support", 4), ("prepared_now", 4), ("sub_rounds", 8), ("undirected_edges", 8), ("triangles", 8),
                      ("support_elements", 8), ("peel_elements", 8), ("algorithmic_bytes", 8)]
    assert ctypes.sizeof(lib.KtrussStats) == 64                                  # the int32 fields first, then the int64 fields: no padding holes
    assert os.path.exists(os.path.join(ROOT, "apps", "bin", "ktruss_hip"))
