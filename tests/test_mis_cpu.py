"""CPU tests of the maximal independent set / maximal matching contract: the restatement (tests/mis_reference.py) on hand-made cases with the expected
sets written out, the sequential definition against the synchronous rounds, the properties against networkx, the closed form of the rounds, and the
C ABI (include/vgl_hip.h declares the four entry points, the ctypes table has them and the structs, the api has the functions)."""
import ctypes
import os
import re

import numpy as np
import pytest

import mis_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_graph(seed):
    rng = np.random.default_rng(seed)
    V = int(rng.integers(1, 121))
    E = int(rng.integers(0, 4 * V + 1))
    G = R.simple_graph(V, rng.integers(0, V, E), rng.integers(0, V, E))
    few = seed % 3 == 0                                                          # every third graph: priorities from a handful of values, ties abound
    vprio = rng.integers(0, 4 if few else 1 << 32, V).astype(np.uint64)
    eprio = rng.integers(0, 4 if few else 1 << 32, G["eu"].size).astype(np.uint64)
    return G, vprio, eprio


def test_key_is_the_headers_and_a_bijection():
    def fmix(h):
        h ^= h >> 16
        h = h * 0x85ebca6b & 0xFFFFFFFF
        h ^= h >> 13
        h = h * 0xc2b2ae35 & 0xFFFFFFFF
        return h ^ h >> 16
    for seed in (0, 7, 0xFFFFFFFF):
        mix = fmix((seed + 0x9e3779b9) & 0xFFFFFFFF)
        for i in (0, 1, 2, 12345, 0x7FFFFFFF, 0xFFFFFFFF):
            assert int(R.key([i], seed)[0]) == fmix(i ^ mix), (seed, i)
    assert fmix(0) == 0 and fmix(1) == 0x514e28b7                                # the murmur3 finaliser's known values
    k = R.key(np.arange(1 << 20), 7)
    assert np.unique(k).size == 1 << 20 and int(k.max()) <= 0xFFFFFFFF


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_restatement_equals_hand_cases(name):
    G, vprio, eprio, in_set, mask = R.hand_case(name)
    assert np.array_equal(R.greedy_mis_sequential(G, vprio), in_set), name
    m = R.mis_rounds(G, vprio)
    assert np.array_equal(m["in_set"], in_set) and m["set_size"] == int(in_set.sum()), name
    got, mate = R.greedy_matching_sequential(G, eprio)
    assert np.array_equal(got, mask), name
    mm = R.matching_rounds(G, eprio)
    assert np.array_equal(mm["in_matching"], mask) and np.array_equal(mm["mate"], mate) and mm["matched_edges"] == int(mask.sum()), name
    if G["V"] == 0:
        assert m["rounds"] == mm["rounds"] == m["live_total"] == mm["live_total"] == 0


def test_rounds_of_the_hand_cases():
    rounds = {name: (R.mis_rounds(*R.hand_case(name)[:2])["rounds"], R.matching_rounds(R.hand_case(name)[0], R.hand_case(name)[2])["rounds"]) for name in R.HAND_CASES}
    assert rounds == {"empty": (0, 0), "isolated_vertices": (1, 1), "only_loops": (1, 1), "one_edge_stored_three_times": (2, 1), "path_6": (2, 2), "cycle_6": (5, 3),
                      "k5": (2, 3), "star_8": (2, 2), "k33": (2, 2), "bowtie": (4, 2)}       # (worked out by hand from the rules of the contract)


@pytest.mark.parametrize("seed", range(60))
def test_sequential_equals_rounds(seed):
    G, vprio, eprio = _random_graph(seed)
    m = R.mis_rounds(G, vprio)
    assert np.array_equal(m["in_set"], R.greedy_mis_sequential(G, vprio))
    mask, mate = R.greedy_matching_sequential(G, eprio)
    mm = R.matching_rounds(G, eprio)
    assert np.array_equal(mm["in_matching"], mask) and np.array_equal(mm["mate"], mate)
    assert m["live_total"] >= G["V"] and m["entries_walked"] >= G["adj"].size and mm["live_total"] >= G["V"] and mm["entries_walked"] >= G["adj"].size
    # default keys too
    assert np.array_equal(R.mis_rounds(G, R.key(np.arange(G["V"]), seed))["in_set"], R.greedy_mis_sequential(G, R.key(np.arange(G["V"]), seed)))


@pytest.mark.parametrize("seed", range(30))
def test_properties_against_networkx(seed):
    nx = pytest.importorskip("networkx")
    G, vprio, eprio = _random_graph(seed)
    X = nx.Graph()
    X.add_nodes_from(range(G["V"]))
    X.add_edges_from(zip(G["eu"].tolist(), G["ev"].tolist()))
    chosen = set(np.flatnonzero(R.mis_rounds(G, vprio)["in_set"]).tolist())
    assert not any(a in chosen and b in chosen for a, b in X.edges())                            # independent
    assert all(v in chosen or any(w in chosen for w in X[v]) for v in X.nodes())                 # maximal
    mm = R.matching_rounds(G, eprio)
    matching = {(int(G["eu"][e]), int(G["ev"][e])) for e in np.flatnonzero(mm["in_matching"])}
    assert nx.is_maximal_matching(X, matching)
    cover = set(np.flatnonzero(mm["mate"] >= 0).tolist())
    assert all(a in cover or b in cover for a, b in X.edges()) and len(cover) == 2 * len(matching)
    assert all(mm["mate"][mm["mate"][v]] == v for v in cover)


@pytest.mark.parametrize("seed", range(30))
def test_round_closed_form(seed):
    """round(IN v) = 1 + max |round(w)| over the neighbours before v (1 without any); round(OUT v) = 1 + min round(w) over the IN neighbours before v"""
    G, vprio, _ = _random_graph(seed)
    rnd = R.mis_rounds(G, vprio)["round"].astype(np.int64)
    _, rank = R._rank(vprio)
    assert bool((rnd != 0).all())
    for v in range(G["V"]):
        nb = G["adj"][G["rowptr"][v]:G["rowptr"][v + 1]]
        nb = nb[rank[nb] < rank[v]]
        if rnd[v] > 0:
            assert rnd[v] == 1 + (int(np.abs(rnd[nb]).max()) if nb.size else 0) and bool((rnd[nb] < 0).all())
        else:
            assert -rnd[v] == 1 + int(rnd[nb][rnd[nb] > 0].min())


def test_team_edge_graph_fills_the_classes_as_it_says():
    """the graph of the GPU test of the kernels' item-count edges: 33 / 5 / 2 rows per class, row lengths on the bounds"""
    V, src, dst = R.rows_at_the_team_edges()
    shrt, wave = R.TEAM_EDGE_BOUNDS
    deg = R.simple_graph(V, src, dst)["deg"]
    cls = np.where(deg <= shrt, 0, np.where(deg <= wave, 1, 2))
    assert tuple(np.bincount(cls, minlength=3).tolist()) == R.TEAM_EDGE_ROWS == (33, 5, 2)
    assert 33 == 32 + 1 and 5 == 4 + 1                                           # a full workgroup of 8-lane teams, of wavefronts, and one more
    for want in (0, shrt, shrt + 1, wave, wave + 1):
        assert (deg == want).any(), (want, deg.tolist())
    assert deg[7] == 0 and deg.max() <= V - 1


def test_path_64_closed_forms():
    G = R.simple_graph(64, np.arange(63), np.arange(1, 64))
    m = R.mis_rounds(G, np.arange(64))
    assert m["rounds"] == 64 and np.array_equal(m["round"], np.where(np.arange(64) % 2 == 0, 1, -1) * (np.arange(64) + 1))
    mm = R.matching_rounds(G, np.arange(63))
    assert mm["rounds"] == 32 and mm["matched_edges"] == 32 and np.array_equal(mm["round"], np.arange(64) // 2 + 1)
    assert np.array_equal(mm["mate"], np.arange(64) ^ 1)


def test_bytes_model_is_the_headers():
    assert R.algorithmic_bytes("mis", 10, 14, 25, 40, 3) == 12 * 10 + 24 * 25 + 8 * 40 + 64 * 4 + 5 * 10
    assert R.algorithmic_bytes("mis", 10, 14, 25, 40, 3, in_set=False) == 12 * 10 + 24 * 25 + 8 * 40 + 64 * 4
    assert R.algorithmic_bytes("matching", 10, 14, 25, 40, 3) == 20 * 10 + 28 * 25 + 12 * 40 + 72 * 4 + 16 * 7 + 7 + 4 * 10
    assert R.algorithmic_bytes("matching", 10, 14, 25, 40, 3, edges=False, in_matching=False, round=False) == 20 * 10 + 28 * 25 + 12 * 40 + 72 * 4
    assert R.algorithmic_bytes("mis", 0, 0, 0, 0, 0) == R.algorithmic_bytes("matching", 0, 0, 0, 0, 0) == 0


def test_header_declares_and_binding_has_the_entry_points():
    text = open(os.path.join(ROOT, "include", "vgl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+vgl_hip_mis_prepare\s*\(\s*vgl_hip_ctx\s*\*\s*\w+\s*,\s*vgl_hip_graph\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+vgl_hip_mis_run\s*\([^;]*const\s+uint32_t\s*\*\s*d_priority\s*,\s*uint32_t\s+seed[^;]*uint8_t\s*\*\s*d_in_set[^;]*int32_t\s*\*\s*d_round"
                     r"[^;]*vgl_hip_mis_stats\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+vgl_hip_matching_prepare\s*\(\s*vgl_hip_ctx\s*\*\s*\w+\s*,\s*vgl_hip_graph\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+vgl_hip_matching_run\s*\([^;]*const\s+uint32_t\s*\*\s*d_edge_priority\s*,\s*uint32_t\s+seed[^;]*int32_t\s*\*\s*d_edge_u[^;]*int32_t\s*\*\s*d_edge_v"
                     r"[^;]*uint8_t\s*\*\s*d_in_matching[^;]*int32_t\s*\*\s*d_mate[^;]*int32_t\s*\*\s*d_round[^;]*vgl_hip_matching_stats\s*\*\s*\w+\s*\)\s*;", text)
    from vectorgraphlibrary_amd import api, lib
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    want = {"mis": [("int32_t", "rounds"), ("int32_t", "prepared_now"), ("int64_t", "set_size"), ("int64_t", "live_total"), ("int64_t", "entries_walked"),
                    ("int64_t", "algorithmic_bytes")],
            "matching": [("int32_t", "rounds"), ("int32_t", "prepared_now"), ("int64_t", "matched_edges"), ("int64_t", "matched_vertices"), ("int64_t", "undirected_edges"),
                         ("int64_t", "live_total"), ("int64_t", "entries_walked"), ("int64_t", "algorithmic_bytes")]}
    for name, cls in (("mis", lib.MisStats), ("matching", lib.MatchingStats)):
        struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*vgl_hip_%s_stats\s*;" % name, text)
        assert struct, name
        assert re.findall(r"\b(int32_t|int64_t|double)\s+(\w+)\s*;", struct.group(1)) == want[name]
        assert cls._fields_ == [(n, ctype[t]) for t, n in want[name]]
        assert ctypes.sizeof(cls) == 8 + 8 * (len(want[name]) - 2)                # the two int32 fields first, then the 64-bit fields: no padding holes
    for s in ("vgl_hip_mis_prepare", "vgl_hip_mis_run", "vgl_hip_matching_prepare", "vgl_hip_matching_run"):
        assert s in lib.EXPORTED_SYMBOLS, s
    for f in ("maximal_independent_set", "maximal_matching", "vertex_cover", "priority_key"):
        assert callable(getattr(api, f)), f
    assert callable(api.Graph.prepare_mis) and callable(api.Graph.prepare_matching)
    slots = re.findall(r"\b(?:mis|mm)_[a-z_]+\b", open(os.path.join(ROOT, "include", "vgl_hip.h")).read())
    for s in ("mis_init", "mis_short", "mis_wave", "mis_wg", "mis_publish", "mis_finish", "mm_init", "mm_best_short", "mm_best_wave", "mm_best_wg", "mm_match", "mm_publish"):
        assert s in slots, s


def test_api_key_equals_the_restatement():
    torch = pytest.importorskip("torch")
    from vectorgraphlibrary_amd import api
    ids = np.concatenate([np.arange(1000), [0x7FFFFFFF, 0xFFFFFFFF]])
    for seed in (0, 7, 0xFFFFFFFF):
        assert np.array_equal(api.priority_key(torch.tensor(ids, dtype=torch.int64), seed).numpy().astype(np.uint64), R.key(ids, seed))


def test_built_library_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from vectorgraphlibrary_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    for s in ("vgl_hip_mis_prepare", "vgl_hip_mis_run", "vgl_hip_matching_prepare", "vgl_hip_matching_run"):
        assert hasattr(L, s), s
    assert os.path.exists(os.path.join(ROOT, "apps", "bin", "mis_hip"))
