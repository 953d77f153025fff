"""CPU proof that the references of tests/test_sssp_weights_gpu.py deserve to be trusted on adversarial weights: for every weight class and graph,
the oracle's Bellman-Ford, the oracle's Dijkstra and a plain numpy restatement agree in every bit (and the three widest-path counterparts do), and
the cases are not vacuous: at least half of the vertices are reached.  No GPU."""
import numpy as np
import pytest

import sssp_weights_reference as R

_CACHE = {}


def _case(O, g):
    if g["name"] not in _CACHE:
        rowptr, adj, perm = O.coo_to_csr(g["V"], g["src"], g["dst"])
        source = O.pick_source(rowptr, g["seed"])
        levels, _ = O.bfs_top_down(rowptr, adj, source)
        _CACHE[g["name"]] = (rowptr, adj, perm, source, levels)
    return _CACHE[g["name"]]


def _all_graphs(O):
    return {g["name"]: g for g in R.graphs(O) + R.small_graphs(O) + [R.block_pair_graph(O)]}


MAIN = ["rmat_s12_e16", "ru_s13_e8", "ring_300"]
OTHERS = ["ring_1024", "rmat_s10_e8", "rmat_s15_e16"]


def test_graph_lists_are_the_named_ones(oracle):
    assert [g["name"] for g in R.graphs(oracle)] == MAIN
    assert [g["name"] for g in R.small_graphs(oracle)] + [R.block_pair_graph(oracle)["name"]] == OTHERS


@pytest.mark.parametrize("gname", MAIN + OTHERS)
@pytest.mark.parametrize("cls", sorted(R.WEIGHT_CLASSES))
def test_three_shortest_path_references_agree(cls, gname, oracle):
    O = oracle
    g = _all_graphs(O)[gname]
    rowptr, adj, perm, source, levels = _case(O, g)
    w = R.make(R.WEIGHT_CLASSES, cls, len(g["src"]), g["seed"])[perm]
    bf, _ = O.sssp_bellman_ford(rowptr, adj, w, source)
    dj = O.sssp_dijkstra(rowptr, adj, w, source)
    nd = R.sssp_numpy(g["V"], R.csr_sources(rowptr), adj, w, source)
    reached = bf < R.FLT_MAX
    print("sssp %-14s %-13s reached %.3f of %d vertices" % (cls, gname, reached.mean(), g["V"]))
    assert (bf.view(np.int32) == dj.view(np.int32)).all(), "Bellman-Ford != Dijkstra"
    assert (bf.view(np.int32) == nd.view(np.int32)).all(), "Bellman-Ford != numpy restatement"
    assert (reached == (levels > 0)).all() and bf[source] == 0.0
    assert reached.mean() >= 0.5, "vacuous case: fewer than half of the vertices are reached"
    if cls == "ones":
        assert (bf[reached] == (levels[reached] - 1).astype(np.float32)).all()          # BFS levels start at 1
    if cls == "zeros":
        assert (bf[reached] == 0.0).all()
    if cls == "wide_range":
        assert np.isfinite(bf[reached]).all() and (bf[reached] < R.FLT_MAX).all()       # "sums stay finite"
    if cls == "denormals":
        assert (bf[reached] < np.finfo(np.float32).tiny).any()                          # the result itself holds denormals


@pytest.mark.parametrize("gname", MAIN + OTHERS)
@pytest.mark.parametrize("cls", sorted(R.CAPACITY_CLASSES))
def test_three_widest_path_references_agree(cls, gname, oracle):
    O = oracle
    g = _all_graphs(O)[gname]
    rowptr, adj, perm, source, levels = _case(O, g)
    cap = R.make(R.CAPACITY_CLASSES, cls, len(g["src"]), g["seed"])[perm]
    bf, _ = O.sswp_bellman_ford(rowptr, adj, cap, source)
    sq = O.sswp_seq(rowptr, adj, cap, source)
    nw = R.sswp_numpy(g["V"], R.csr_sources(rowptr), adj, cap, source)
    positive = (bf > 0).mean()
    print("sswp %-14s %-13s width > 0 on %.3f of %d vertices (reached %.3f)" % (cls, gname, positive, g["V"], (levels > 0).mean()))
    assert (bf.view(np.int32) == sq.view(np.int32)).all(), "Bellman-Ford != worklist"
    assert (bf.view(np.int32) == nw.view(np.int32)).all(), "Bellman-Ford != numpy restatement"
    assert bf[source] == R.FLT_MAX and (bf[levels < 0] == 0).all()
    assert (levels > 0).mean() >= 0.5, "vacuous case: fewer than half of the vertices are reached"
    if cls == "zeros":
        others = np.arange(g["V"]) != source
        assert (bf[others] == 0).all()
    if cls == "ones":
        others = (levels > 0) & (np.arange(g["V"]) != source)
        assert (bf[others] == 1.0).all()
    if cls == "flt_max_some" and gname in MAIN[:2]:                                    # (where the source has tens of outgoing edges)
        assert (bf[np.arange(g["V"]) != source] == R.FLT_MAX).any()                    # a vertex other than the source at FLT_MAX: a legal result


# (class, delta variant of the GPU tests) whose delta EQUALS many weights
ON_THE_BOUNDARY = [("two_values", "16"), ("small_ints", "max"), ("small_ints", "min_positive"), ("ones", "max"), ("top_of_domain", "max")]


@pytest.mark.parametrize("gname", MAIN)
@pytest.mark.parametrize("cls,variant", ON_THE_BOUNDARY)
def test_weights_equal_to_delta_decide_distances(cls, variant, gname, oracle):
    """the boundary cases of the GPU tests are not vacuous: a plan whose partition placed edges by w <= delta while its flags say w < delta (the
    first seeded mistake of the sensitivity check, modelled on the host) ends at other distances than the reference, whichever way its write
    collisions go -- so the bit comparison of the delta-stepping runs depends on the edges with w == delta.  The true plan is a permutation
    of the edges and ends at the reference."""
    O = oracle
    g = _all_graphs(O)[gname]
    rowptr, adj, perm, source, levels = _case(O, g)
    w = R.make(R.WEIGHT_CLASSES, cls, len(g["src"]), g["seed"])[perm]
    delta = {"16": np.float32(16.0), "max": w.max(), "min_positive": w[w > 0].min()}[variant]
    assert (w == delta).sum() >= len(w) // 8
    bf, _ = O.sssp_bellman_ford(rowptr, adj, w, source)
    true_plan = R.sssp_numpy(g["V"], *R.delta_plan_edges(rowptr, adj, w, delta), source)
    assert (true_plan.view(np.int32) == bf.view(np.int32)).all()
    for first in (False, True):
        wrong = R.sssp_numpy(g["V"], *R.delta_plan_edges(rowptr, adj, w, delta, place_le=True, first_writer_wins=first), source)
        differing = int((wrong.view(np.int32) != bf.view(np.int32)).sum())
        print("%s %s delta %s: %d edges on the boundary, %d distances differ" % (cls, gname, variant, int((w == delta).sum()), differing))
        assert differing > 0
