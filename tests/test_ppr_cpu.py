"""The restatement of the personalised-PageRank contract (tests/ppr_reference.py) pinned on the CPU before tests/test_ppr_gpu.py compares the HIP
kernels with it: against the dense solve the iteration converges to, against networkx on a MultiDiGraph, against closed forms, and its invariants.
Every bound is the derived tolerance (ppr_reference.tolerance) plus what the other side of the comparison is known to be off by."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppr_reference as R  # noqa: E402

ALPHA = 0.85
T = 400                     # 2 alpha^T = 1.2e-28: the iteration has converged as far as float64 can tell


def l1(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).sum())


def solve_with_its_error(G, p, alpha):
    """x* and a bound on its own L1 error: |r|_1 / (1 - alpha) for the residual r, since T = M + p dang^T has column sums 1 and so
    |(I - alpha T)^-1|_1 <= 1 / (1 - alpha)"""
    x = R.dense_solve(G, p, alpha)
    inv = np.where(G.dangling, 0.0, 1.0 / np.maximum(G.outdeg, 1))
    Tm = G.AT.toarray() * inv[None, :] + np.outer(p, G.dangling.astype(np.float64))
    r = (1.0 - alpha) * p - (x - alpha * (Tm @ x))
    return x, float(np.abs(r).sum()) / (1.0 - alpha)


def seed_cases(V):
    return [([0], None), ([V - 1, 1, V // 2], [3.0, 1.0, 0.5]), ([2, 2, 1], [1.0, 2.0, 1.0]), ([], None)]


@pytest.fixture(scope="module")
def rmat10(oracle):
    src, dst = oracle.gen_rmat(10, 8, 2)
    return R.Graph(1 << 10, src, dst)


def check_dense(G, what):
    lists = [s for s, _ in seed_cases(G.V)]
    weights = [w for _, w in seed_cases(G.V)]
    rank, err, its, st = R.pagerank(G, lists, weights, ALPHA, T)
    assert st["batches"] == 1 and list(its) == [T] * len(lists)
    for j, (s, w) in enumerate(seed_cases(G.V)):
        p = R.teleport(G.V, s, w)
        want, own = solve_with_its_error(G, p, ALPHA)
        bound = R.tolerance(G.d_max, G.n_dangling, ALPHA, T) + 2.0 * ALPHA ** T + own
        d = l1(rank[j], want)
        print(what, "seeds", s, "L1 to the dense solve", d, "bound", bound, "of which the solve", own)
        assert d <= bound
        assert err[j] <= 2.0 * R.tolerance(G.d_max, G.n_dangling, ALPHA, T) + 4.0 * ALPHA ** (T - 1)


@pytest.mark.parametrize("name", list(R.SMALL))
def test_dense_solve_on_small_graphs(name):
    check_dense(R.Graph(*R.small(name)), name)


def test_dense_solve_on_rmat(rmat10):
    assert rmat10.n_dangling > 0 and rmat10.d_max > 64
    check_dense(rmat10, "rmat 10 x 8")


@pytest.mark.parametrize("personalised", [False, True])
def test_networkx_multidigraph(personalised, rmat10):
    nx = pytest.importorskip("networkx")
    G = rmat10
    coo = G.A.tocoo()
    M = nx.MultiDiGraph()
    M.add_nodes_from(range(G.V))
    for a, b, m in zip(coo.row.tolist(), coo.col.tolist(), coo.data.tolist()):
        M.add_edges_from([(a, b)] * int(m))
    assert M.number_of_edges() == G.E
    seeds, weights = ([5, 900, 33], [2.0, 1.0, 4.0]) if personalised else ([], None)
    tol_nx = 1e-13
    want = nx.pagerank(M, alpha=ALPHA, personalization=dict(zip(seeds, weights)) if personalised else None, max_iter=1000, tol=tol_nx)
    want = np.array([want[v] for v in range(G.V)])
    rank, _, _, _ = R.pagerank(G, [seeds], None if weights is None else [weights], ALPHA, T)
    # networkx stops at an L1 change below N tol, alpha / (1 - alpha) times which bounds its distance to the fixed point; its float64 sums run in
    # another order for an unknown number of iterations: the tolerance's limit gamma_k / (1 - alpha)
    inf = R.tolerance(G.d_max, G.n_dangling, ALPHA, 10 ** 6)
    bound = R.tolerance(G.d_max, G.n_dangling, ALPHA, T) + inf + 2.0 * ALPHA ** T + ALPHA / (1.0 - ALPHA) * G.V * tol_nx
    d = l1(rank[0], want)
    print("personalised", personalised, "L1 to networkx", d, "bound", bound)
    assert d <= bound


@pytest.mark.parametrize("n", [3, 7, 50])
def test_cycle_and_path_closed_form(n):
    """a directed n-cycle with one seed: x[k] = (1 - alpha) alpha^k / (1 - alpha^n) at distance k; a path that ends in a dangling vertex hands that
    vertex's mass back to the seed, which is the same chain"""
    want = (1.0 - ALPHA) * ALPHA ** np.arange(n) / (1.0 - ALPHA ** n)
    cycle = R.Graph(n, np.arange(n), (np.arange(n) + 1) % n)
    path = R.Graph(n, np.arange(n - 1), np.arange(1, n))
    assert cycle.n_dangling == 0 and path.n_dangling == 1
    for G, seed in ((cycle, 2), (path, 0)):
        rank, _, _, _ = R.pagerank(G, [[seed]], None, ALPHA, T)
        bound = R.tolerance(1, G.n_dangling, ALPHA, T) + 2.0 * ALPHA ** T + 8 * R.U        # the closed form's own roundings: a power, two differences, a quotient
        assert l1(np.roll(rank[0], -seed), want) <= bound


def test_complete_graph_uniform():
    V, src, dst = R.small("complete")
    G = R.Graph(V, src, dst)
    rank, err, _, _ = R.pagerank(G, [[]], None, ALPHA, 50)
    assert l1(rank[0], np.full(V, 1.0 / V)) <= R.tolerance(G.d_max, 0, ALPHA, 50)


@pytest.mark.parametrize("name", list(R.SMALL))
def test_invariants(name):
    V, src, dst = R.small(name)
    G = R.Graph(V, src, dst)
    cases = seed_cases(V)
    lists, weights = [s for s, _ in cases], [w for _, w in cases]
    p = [R.teleport(V, s, w) for s, w in cases]
    for j, q in enumerate(p):
        total = np.float64(0.0)
        for x in q:
            total = total + x
        assert abs(total - 1.0) <= V * R.U and (q >= 0).all()
    assert p[2][2] == 0.75 and p[2][1] == 0.25                              # a vertex listed twice gets both weights
    for t in (0, 1, 3, 50):
        rank, err, its, _ = R.pagerank(G, lists, weights, ALPHA, t)
        tol = R.tolerance(G.d_max, G.n_dangling, ALPHA, t)
        assert (rank >= 0).all() and list(its) == [t] * len(cases)
        for j in range(len(cases)):
            assert abs(rank[j].sum() - 1.0) <= tol + V * R.U, (name, t, j)      # mass 1 (the check's own sum: V roundings)
            if t == 0:
                assert np.array_equal(rank[j], p[j]) and err[j] == 0.0
            if lists[j]:
                assert np.array_equal(rank[j] != 0, R.support(G, lists[j], t)), (name, t, j)
    rank, _, _, _ = R.pagerank(G, lists, weights, 0.0, 5)                    # alpha = 0 returns p exactly
    for j in range(len(cases)):
        assert np.array_equal(rank[j], p[j])


def test_batches_stop_together(rmat10):
    G = rmat10
    lists = [[v] for v in range(20)] + [[]]
    rank, err, its, st = R.pagerank(G, lists, None, ALPHA, 200, tol=1e-9)
    assert st["batches"] == 2 and st["batches_converged"] == 2 and st["sources"] == 21
    assert len(set(its[:16])) == 1 and len(set(its[16:])) == 1 and st["iterations_total"] == int(its[0]) + int(its[16])
    assert st["entries_walked"] == st["iterations_total"] * G.E and st["max_err"] == err.max() <= 1e-9
    for j in (0, 15, 16, 20):
        want, own = solve_with_its_error(G, R.teleport(G.V, lists[j]), ALPHA)
        assert l1(rank[j], want) <= ALPHA * err[j] / (1.0 - ALPHA) + R.tolerance(G.d_max, G.n_dangling, ALPHA, int(its[j])) + own


def test_the_tolerance_itself():
    """the worked figure of DESIGN section 28: d_max 212, 327 dangling vertices, alpha 0.85, 50 iterations"""
    assert 2.4e-13 < R.tolerance(212, 327, 0.85, 50) < 2.5e-13
    assert R.tolerance(5, 0, 0.5, 0) == 0.0 and R.tolerance(5, 0, 0.0, 3) == 11 * R.U / (1 - 11 * R.U)
