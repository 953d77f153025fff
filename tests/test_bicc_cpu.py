"""CPU tests of the biconnectivity contract: the sequential restatement (tests/bicc_reference.py) on hand-made cases with the expected values written
out, against networkx (bridges, articulation_points, biconnected_component_edges, k_edge_components), the by-construction counts of block_graph, and
the C ABI (include/vgl_hip.h declares the two entry points, the ctypes table has them and the struct, the api has the four functions)."""
import ctypes
import os
import re

import numpy as np
import pytest

import bicc_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_GRAPHS = [(1, 300, 0.0), (2, 300, 0.3), (3, 1000, 0.05)]
ARRAYS = ("bridge", "edge_component", "articulation", "two_edge_component")


def _stored(name):
    V, stored, want = R.HAND_CASES[name]
    return V, [a for a, _ in stored], [b for _, b in stored], stored, want


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_restatement_equals_hand_cases(name):
    V, src, dst, stored, want = _stored(name)
    m = R.biconnected(V, src, dst)
    edges = list(zip(m["edge_u"].tolist(), m["edge_v"].tolist()))
    assert edges == sorted({(min(a, b), max(a, b)) for a, b in stored if a != b}), name
    assert [edges[i] for i in np.flatnonzero(m["bridge"])] == want["bridges"], name
    assert np.flatnonzero(m["articulation"]).tolist() == want["cuts"], name
    blocks = {}
    for i, b in enumerate(m["edge_component"].tolist()):
        blocks.setdefault(b, []).append(edges[i])
    assert sorted(blocks.values()) == want["blocks"] and all(b == min(edges.index(e) for e in es) for b, es in blocks.items()), name
    comps = {}
    for v, c in enumerate(m["two_edge_component"].tolist()):
        comps.setdefault(c, []).append(v)
    assert sorted(comps.values()) == want["two_edge"] and all(c == vs[0] for c, vs in comps.items()), name
    for got, exp in zip((m[k] for k in ARRAYS), R.expected_arrays(V, stored, want)):
        assert got.dtype == exp.dtype and np.array_equal(got, exp), name
    assert m["bridges"] == len(want["bridges"]) and m["articulation_points"] == len(want["cuts"]) and m["biconnected_components"] == len(want["blocks"])
    assert m["two_edge_components"] == len(want["two_edge"]) == m["components"] + m["bridges"]
    assert m["largest_component_edges"] == max([len(b) for b in want["blocks"]] + [0])


def test_depths_of_the_hand_cases():
    depth = {name: R.biconnected(*_stored(name)[:3])["depth"] for name in R.HAND_CASES}
    assert depth == {"empty": 1, "isolated_vertices": 1, "only_loops": 1, "one_edge_stored_three_times": 2, "path_6": 6, "cycle_6": 4, "k5": 2, "bowtie": 3,
                     "barbell": 4, "theta": 4, "ladder_2x5": 6, "binary_tree_4": 5, "cross_edge_below_a_cut_vertex": 4}


def _against_networkx(V, src, dst, what):
    import networkx as nx
    m = R.biconnected(V, src, dst)
    eu, ev = m["edge_u"].tolist(), m["edge_v"].tolist()
    G = nx.Graph()
    G.add_nodes_from(range(V))
    G.add_edges_from(zip(eu, ev))
    assert G.number_of_edges() == m["undirected_edges"], what
    edges = list(zip(eu, ev))
    assert sorted((min(a, b), max(a, b)) for a, b in nx.bridges(G)) == [edges[i] for i in np.flatnonzero(m["bridge"])], what
    assert sorted(nx.articulation_points(G)) == np.flatnonzero(m["articulation"]).tolist(), what
    at = {e: i for i, e in enumerate(edges)}
    want = np.full(len(edges), -1, dtype=np.int64)
    n = 0
    for comp in nx.biconnected_component_edges(G):
        ids = [at[(min(a, b), max(a, b))] for a, b in comp]
        want[ids] = min(ids)
        n += 1
    assert np.array_equal(m["edge_component"], want) and m["biconnected_components"] == n, what
    two = np.full(V, -1, dtype=np.int64)
    for comp in nx.k_edge_components(G, 2):
        two[list(comp)] = min(comp)
    assert np.array_equal(m["two_edge_component"], two), what
    assert m["components"] == nx.number_connected_components(G), what
    depth = 0
    for comp in nx.connected_components(G):
        depth = max(depth, 1 + max(nx.single_source_shortest_path_length(G, min(comp)).values()))
    assert m["depth"] == depth, what
    return m


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_restatement_equals_networkx_on_hand_cases(name):
    pytest.importorskip("networkx")
    V, src, dst, _, _ = _stored(name)
    _against_networkx(V, src, dst, name)


@pytest.mark.parametrize("seed,blocks,hub_share", BLOCK_GRAPHS)
def test_block_graph_counts_by_construction_and_networkx(seed, blocks, hub_share):
    V, src, dst, expect = R.block_graph(seed, blocks, hub_share)
    m = R.biconnected(V, src, dst)
    assert {k: m[k] for k in expect} == expect
    assert expect["biconnected_components"] == blocks and expect["components"] == 6
    pytest.importorskip("networkx")
    _against_networkx(V, src, dst, "block_graph %d" % seed)


@pytest.mark.parametrize("seed", range(40))
def test_restatement_equals_networkx_on_random_graphs(seed):
    pytest.importorskip("networkx")
    rng = np.random.default_rng(seed)
    V = int(rng.integers(2, 201))
    E = int(rng.integers(0, 2 * V + 1))                                         # around the threshold where bridges, cut vertices and a large block coexist
    _against_networkx(V, rng.integers(0, V, E), rng.integers(0, V, E), "random %d" % seed)


def test_bytes_model_is_the_headers():
    assert R.algorithmic_bytes(10, 7, 3) == (92 + 33 + 12) * 10 + (16 + 8) * 14 + (24 + 16 + 1 + 20) * 7 + 104 * 4
    assert R.algorithmic_bytes(10, 7, 3, edges=True, bridge=True, blocks=False, two_edge=False) == 92 * 10 + 16 * 14 + 41 * 7 + 104 * 4


def test_header_declares_and_binding_has_the_entry_points():
    text = open(os.path.join(ROOT, "include", "vgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+vgl_hip_bicc_prepare\s*\(\s*vgl_hip_ctx\s*\*\s*\w+\s*,\s*vgl_hip_graph\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+vgl_hip_bicc_run\s*\([^;]*int32_t\s*\*\s*d_edge_u[^;]*int32_t\s*\*\s*d_edge_v[^;]*uint8_t\s*\*\s*d_bridge[^;]*int32_t\s*\*\s*d_edge_component"
                     r"[^;]*uint8_t\s*\*\s*d_articulation[^;]*int32_t\s*\*\s*d_two_edge_component[^;]*vgl_hip_bicc_stats\s*\*\s*\w+\s*\)\s*;", text)
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*vgl_hip_bicc_stats\s*;", text)
    assert struct
    fields = [("int32_t", "depth"), ("int32_t", "prepared_now"), ("int64_t", "undirected_edges"), ("int64_t", "components"), ("int64_t", "bridges"),
              ("int64_t", "articulation_points"), ("int64_t", "biconnected_components"), ("int64_t", "two_edge_components"),
              ("int64_t", "largest_component_edges"), ("int64_t", "algorithmic_bytes")]
    assert re.findall(r"\b(int32_t|int64_t|double)\s+(\w+)\s*;", struct.group(1)) == fields
    from vectorgraphlibrary_amd import api, lib
    for s in ("vgl_hip_bicc_prepare", "vgl_hip_bicc_run"):
        assert s in lib.EXPORTED_SYMBOLS, s
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    assert lib.BiccStats._fields_ == [(n, ctype[t]) for t, n in fields]
    assert ctypes.sizeof(lib.BiccStats) == 72                                    # the two int32 fields first, then the 64-bit fields: no padding holes
    for f in ("biconnected_components", "bridges", "articulation_points", "two_edge_connected_components"):
        assert callable(getattr(api, f)), f


def test_built_library_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from vectorgraphlibrary_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    for s in ("vgl_hip_bicc_prepare", "vgl_hip_bicc_run"):
        assert hasattr(L, s), s
    assert os.path.exists(os.path.join(ROOT, "apps", "bin", "bicc_hip"))
