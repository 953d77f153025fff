"""CPU tests of the k-core contract: the numpy / scipy restatement (tests/kcore_reference.py) against closed forms and networkx.core_number, the k_limit
rule, and the C ABI (include/vgl_hip.h declares the two entry points and the built library exports them)."""
import ctypes
import os
import re

import numpy as np
import pytest

import kcore_reference as R
from tri_reference import simple_undirected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_restatement_equals_closed_forms(name):
    V, edges, want = R.HAND_CASES[name]
    src, dst = zip(*edges)
    core, degree, E, distinct = R.core_numbers(V, src, dst)
    assert core.dtype == np.int32 and degree.dtype == np.int32
    assert core.tolist() == want, name
    assert distinct == len(set(want))
    A = simple_undirected(V, src, dst)
    assert E == A.nnz // 2 and degree.tolist() == np.asarray(A.sum(axis=1)).ravel().tolist()
    assert bool((core <= degree).all())


def _random_graph(rng, V, E, skew):
    if skew:                                     # a few heavy vertices: a dense core over a sparse fringe
        p = 1.0 / np.arange(1, V + 1) ** 0.8
        p /= p.sum()
        src, dst = rng.choice(V, E, p=p), rng.choice(V, E, p=p)
    else:
        src, dst = rng.integers(0, V, E), rng.integers(0, V, E)
    return src.astype(np.int64), dst.astype(np.int64)


@pytest.mark.parametrize("V,E,skew,seed", [(2000, 6000, False, 1), (3000, 30000, True, 2), (4000, 40000, False, 3), (2500, 50000, True, 4)])
def test_restatement_equals_networkx(V, E, skew, seed):
    import networkx as nx
    src, dst = _random_graph(np.random.default_rng(seed), V, E, skew)          # loops and duplicates included: the contract drops them
    core, degree, Eu, distinct = R.core_numbers(V, src, dst)
    A = simple_undirected(V, src, dst).tocoo()                                 # networkx refuses self-loops: it gets the simple graph
    G = nx.Graph()
    G.add_nodes_from(range(V))
    G.add_edges_from(zip(A.row.tolist(), A.col.tolist()))
    assert G.number_of_edges() == Eu
    want = nx.core_number(G)
    assert core.tolist() == [want[v] for v in range(V)]
    assert distinct == len(set(want.values()))


def test_k_limit_is_the_minimum():
    src, dst = _random_graph(np.random.default_rng(7), 3000, 30000, True)
    core, degree, E, distinct = R.core_numbers(3000, src, dst)
    top = int(core.max())
    assert top >= 4
    for k_limit in (1, 3, top, top + 5):
        c, d, e, n = R.core_numbers(3000, src, dst, k_limit)
        assert np.array_equal(c, np.minimum(core, k_limit)) and np.array_equal(d, degree) and e == E
        assert n == np.unique(core[core < k_limit]).size


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "vgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+vgl_hip_kcore_prepare\s*\(\s*vgl_hip_ctx\s*\*\s*\w+\s*,\s*vgl_hip_graph\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+vgl_hip_kcore_run\s*\([^;]*int32_t\s+k_limit[^;]*int32_t\s*\*\s*d_core[^;]*vgl_hip_kcore_stats\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\}\s*vgl_hip_kcore_stats\s*;", text)
    import __graft_entry__ as ge
    ge.build()
    from vectorgraphlibrary_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    for s in ("vgl_hip_kcore_prepare", "vgl_hip_kcore_run"):
        assert hasattr(L, s), s
        assert s in lib.EXPORTED_SYMBOLS
    fields = [n for n, _ in lib.KcoreStats._fields_]
    assert fields == ["degeneracy", "rounds", "max_degree", "prepared_now", "sub_rounds", "undirected_edges", "edges_examined", "algorithmic_bytes"]
    assert ctypes.sizeof(lib.KcoreStats) == 48
