"""The restatement of the louvain contract (tests/louvain_reference.py) pinned against a brute force over Python dicts and ints, closed forms, the
level invariants and networkx; the library's symbols.  No GPU."""
import itertools

import numpy as np
import pytest

import louvain_reference as R
import quotient_reference as QR


def fmix32(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85ebca6b) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def brute_move(rowptr, adj, w=None, max_rounds=64, D=0, seed=0):
    """the contract of include/vgl_hip.h read line by line, one vertex and one entry at a time, Python ints only"""
    V = len(rowptr) - 1
    rows = [[(int(adj[e]), 1 if w is None else int(w[e])) for e in range(int(rowptr[v]), int(rowptr[v + 1]))] for v in range(V)]
    k = [sum(x for _, x in row) for row in rows]
    m = sum(k)
    comm = list(range(V))
    kept, n_kept, n_before, applied, r = comm, 0, 0, 0, 0
    while True:
        r += 1
        tot, size = [0] * V, [0] * V
        for v in range(V):
            tot[comm[v]] += k[v]
            size[comm[v]] += 1
        best, inside = [None] * V, 0
        for v in range(V):
            A = comm[v]
            kvc = {A: 0}
            for far, x in rows[v]:
                if far == v:
                    inside += x
                else:
                    kvc[comm[far]] = kvc.get(comm[far], 0) + x
            inside += kvc[A]
            score = {c: kvc[c] * m - k[v] * (tot[c] - (k[v] if c == A else 0)) for c in kvc}
            top = max(score.values())
            b = min(c for c in score if score[c] == top)
            if b != A and score[b] > score[A] and not (size[A] == 1 and size[b] == 1 and b > A):
                best[v] = b
        W = sum(x is not None for x in best)
        N = m * inside - sum(t * t for t in tot)
        if r > 1 and applied > 0 and N <= n_kept:
            return kept, "reverted", r, n_kept, m
        kept, n_before, n_kept = comm, n_kept, N
        if D > 0 and r > 1 and applied > 0 and N - n_before < (m * m) // D:
            return comm, "small_gain", r, N, m
        if W == 0:
            return comm, "converged", r, N, m
        if r == max_rounds:
            return comm, "capped", r, N, m
        mix = fmix32(seed + r + 0x9e3779b9)
        nxt = list(comm)
        applied = 0
        for v in range(V):
            if best[v] is not None and fmix32(v ^ mix) & 1:
                nxt[v] = best[v]
                applied += 1
        comm = nxt


def assert_move_equals_brute(rowptr, adj, w, max_rounds=64, D=0, seed=0, what=None):
    labels, info = R.move(rowptr, adj, w, max_rounds, D, seed)
    b_labels, b_outcome, b_rounds, b_n, b_m = brute_move(rowptr, adj, w, max_rounds, D, seed)
    assert labels.tolist() == list(b_labels), what
    assert (info["outcome"], info["rounds"], info["N"], info["m"]) == (b_outcome, b_rounds, b_n, b_m), what
    return info


def test_restatement_equals_brute_force_on_all_graphs_of_5_vertices():
    pairs = list(itertools.combinations(range(5), 2))
    for mask in range(1 << len(pairs)):
        chosen = [p for i, p in enumerate(pairs) if mask >> i & 1]
        src, dst = QR._both(chosen) if chosen else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        rowptr, adj, _ = QR.coo_to_csr(5, src, dst)
        assert_move_equals_brute(rowptr, adj, None, seed=mask & 3, what=mask)


def test_restatement_equals_brute_force_on_random_multigraphs():
    rng = np.random.default_rng(27)
    outcomes = set()
    for trial in range(150):
        V = int(rng.integers(1, 13))
        E = int(rng.integers(0, 4 * V + 1))
        s, d = rng.integers(0, V, size=E), rng.integers(0, V, size=E)
        src, dst = np.concatenate([s, d]).astype(np.int32), np.concatenate([d, s]).astype(np.int32)      # symmetric, with loops and repeats
        rowptr, adj, perm = QR.coo_to_csr(V, src, dst)
        ew = rng.integers(0, 6, size=E)
        w = np.concatenate([ew, ew])[perm].astype(np.int64)
        for weights in (None, w):
            for max_rounds, D in ((64, 0), (3, 0), (64, 50)):
                outcomes.add(assert_move_equals_brute(rowptr, adj, weights, max_rounds, D, seed=trial, what=(trial, max_rounds, D))["outcome"])
    assert outcomes == set(R.OUTCOMES)


def run_on(name, **kw):
    V, src, dst = R.fixed_graphs()[name]
    rowptr, adj, _ = R.simple_graph(V, src, dst)
    return R.run(rowptr, adj, None, **kw)


def test_closed_forms():
    community, levels, st, infos = run_on("one_edge")
    labels, _ = R.move(*R.simple_graph(*R.fixed_graphs()["one_edge"])[:2])
    assert labels.tolist() == [0, 0] and community.tolist() == [0, 0]
    V, src, dst = R.fixed_graphs()["matching16"]
    labels, info = R.move(*R.simple_graph(V, src, dst)[:2])
    assert labels.tolist() == [2 * (v // 2) for v in range(16)] and info["communities"] == 8
    community, _, st, _ = run_on("matching16")
    assert community.tolist() == [v // 2 for v in range(16)]
    community, _, st, _ = run_on("star")
    assert len(set(community.tolist())) == 1
    community, _, st, _ = run_on("caveman")
    assert community.tolist() == [v // 6 for v in range(48)]
    community, levels, st, infos = run_on("empty")
    assert community.tolist() == list(range(5)) and st["levels"] == 1 and st["outcome"] == ["converged"] and st["modularity_num"] == 0 and st["total_weight"] == 0


def outcomes_of(name, **kw):
    return run_on(name, **kw)[2]["outcome"]


def test_every_outcome_on_the_fixed_cases():
    V, src, dst = R.gnp(2000, 0.005, 1)
    st = R.run(*R.simple_graph(V, src, dst)[:2])[2]
    assert st["outcome"][0] == "reverted"
    assert "capped" in outcomes_of("grid12", max_rounds=5)
    assert "small_gain" in outcomes_of("grid12", min_gain_den=20)
    seen = set()
    for name in R.fixed_graphs():
        seen |= set(outcomes_of(name))
    assert "converged" in seen


def test_level_invariants():
    for name in ("caveman", "ring_of_cliques", "petersen", "grid12", "gnp300"):
        for seed in (0, 1):
            community, levels, st, infos = run_on(name, seed=seed)
            for l, info in enumerate(infos):
                judged = [n for n, _, _ in info["trace"]]
                if info["outcome"] == "reverted":
                    judged = judged[:-1]
                kept = [n for i, n in enumerate(judged) if i == 0 or info["trace"][i][2] > 0]
                assert all(a < b for a, b in zip(kept, kept[1:])), (name, l)
                assert info["N"] == kept[-1] >= info["trace"][0][0]
                if l + 1 < len(infos):
                    assert infos[l + 1]["trace"][0][0] == info["N"], (name, l)
            assert st["modularity_num"] == infos[-1]["N"] and st["communities"][-1] == st["vertices"][-1]
            assert len(set(levels[-1].tolist())) == st["communities"][-1] and int(levels[-1].max()) == st["communities"][-1] - 1


def test_weight_limits():
    rowptr, adj = np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int32)
    w = np.array([2 ** 30 - 1, 2 ** 30 - 1], dtype=np.int64)
    info = assert_move_equals_brute(rowptr, adj, w)
    assert info["m"] == 2 ** 31 - 2 and info["outcome"] == "converged"
    with pytest.raises(ValueError):
        R.move(rowptr, adj, w + np.array([1, 1]))
    with pytest.raises(ValueError):
        R.move(rowptr, adj, np.array([1, -1], dtype=np.int64))


def nx_cases(nx):
    return {"karate": nx.karate_club_graph(), "ring_of_cliques": nx.ring_of_cliques(30, 5),
            "planted": nx.planted_partition_graph(16, 32, 0.4, 0.01, seed=1), "gnp": nx.gnp_random_graph(200, 0.05, seed=1), "grid": nx.convert_node_labels_to_integers(nx.grid_2d_graph(30, 30))}


@pytest.mark.parametrize("name", ["karate", "ring_of_cliques", "planted", "gnp", "grid"])
def test_quality_against_networkx(name):
    nx = pytest.importorskip("networkx")
    G = nx_cases(nx)[name]
    V = G.number_of_nodes()
    e = np.array([(a, b) for a, b in G.edges() if a != b], dtype=np.int32)
    rowptr, adj, _ = R.simple_graph(V, np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))
    community, levels, st, infos = R.run(rowptr, adj)
    q = R.modularity(st)
    parts = [set(np.flatnonzero(community == c).tolist()) for c in range(int(community.max()) + 1)]
    assert abs(q - nx.community.modularity(G, parts, weight=None)) <= 1e-12
    theirs = min(nx.community.modularity(G, nx.community.louvain_communities(G, weight=None, seed=s), weight=None) for s in range(5))
    print(name, "Q", q, "networkx least", theirs)
    assert q >= theirs - 0.02


def test_library_exports_the_louvain_symbol():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from vectorgraphlibrary_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "vgl_hip_louvain_move") and "vgl_hip_louvain_move" in lib.EXPORTED_SYMBOLS
    assert ctypes.sizeof(lib.LouvainStats) == 8 + 10 * 8 + 4 * 32 * 8 + 2 * 32 * 4
