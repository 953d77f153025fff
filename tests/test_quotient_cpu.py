"""The restatement of the quotient contract (tests/quotient_reference.py) pinned against an independent brute force, closed forms and the composition
law; no GPU, no library."""
from fractions import Fraction

import numpy as np
import pytest

import quotient_reference as R


def same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_numpy_equals_brute_force_on_the_hand_cases(name):
    V, src, dst = R.hand_cases()[name]
    rowptr, adj, in_rowptr, in_adj = R.build(V, src, dst)
    w = (np.arange(len(adj), dtype=np.int64) * 7 + 3) % 11
    for lname, labels in R.labelings(V).items():
        for rp, ad in ((rowptr, adj), (in_rowptr, in_adj)):
            for drop in (False, True):
                for weights in (None, w):
                    assert same(R.quotient_dir(rp, ad, labels, weights, drop), R.quotient_brute(rp, ad, labels, weights, drop)), (name, lname, drop)


def test_numpy_equals_brute_force_on_random_multigraphs():
    rng = np.random.default_rng(25)
    for trial in range(40):
        V = int(rng.integers(1, 65))
        src, dst = R.random_multigraph(rng, V, int(rng.integers(0, 4 * V + 1)))
        rowptr, adj, in_rowptr, in_adj = R.build(V, src, dst)
        labels = rng.integers(0, int(rng.integers(1, V + 1)), size=V) * int(rng.integers(1, 1000))
        w = rng.integers(-5, 1 << 20, size=len(adj))
        for rp, ad in ((rowptr, adj), (in_rowptr, in_adj)):
            for drop in (False, True):
                got, want = R.quotient_dir(rp, ad, labels, w, drop), R.quotient_brute(rp, ad, labels, w, drop)
                assert same(got, want), trial
                assert all(np.all(np.diff(got[1][got[0][c]:got[0][c + 1]]) > 0) for c in range(len(got[0]) - 1)), trial      # ascending, no repeats


def test_vertex_maps():
    labels = np.array([10, 5, 10, 2 ** 31 - 2, 5, 5], dtype=np.int64)
    cluster_of, label_of, size, members, member_ptr = R.vertex_maps(labels)
    assert cluster_of.tolist() == [1, 0, 1, 2, 0, 0] and label_of.tolist() == [5, 10, 2 ** 31 - 2] and size.tolist() == [3, 2, 1]
    assert members.tolist() == [1, 4, 5, 0, 2, 3] and member_ptr.tolist() == [0, 3, 5, 6]
    perm = np.array([3, 0, 5, 1, 2, 4])                               # the numbering of the coarse vertices follows the label values alone
    assert R.vertex_maps(labels[perm])[1].tolist() == label_of.tolist()


def test_two_cliques_have_modularity_one_half():
    for n in (2, 3, 5, 8):
        V, src, dst = R.two_cliques(n)
        rowptr, adj, _, _ = R.build(V, src, dst)
        labels = (np.arange(V) >= n).astype(np.int64)
        assert R.modularity_fraction(rowptr, adj, labels) == Fraction(1, 2)
        assert R.modularity_fraction(rowptr, adj, np.zeros(V, dtype=np.int64)) == 0
        q = R.quality(rowptr, adj, labels)
        assert q["cut"] == 0 and q["total"] == 2 * n * (n - 1) and q["volume_out"].sum() == q["volume_in"].sum() == q["total"]


def test_one_cluster_has_modularity_zero_and_no_entries_none():
    for name, (V, src, dst) in R.hand_cases().items():
        rowptr, adj, _, _ = R.build(V, src, dst)
        assert R.modularity_fraction(rowptr, adj, np.full(V, 3)) == 0, name
    assert R.modularity_fraction(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), np.arange(3)) == 0


def test_identity_labels_give_the_graph_back():
    rng = np.random.default_rng(7)
    V = 40
    pairs = np.unique(rng.integers(0, V, size=(300, 2)), axis=0)      # sorted unique COO
    rowptr, adj, _, _ = R.build(V, pairs[:, 0], pairs[:, 1])
    rp, ad, cnt = R.quotient_dir(rowptr, adj, np.arange(V) * 3 + 1)
    assert np.array_equal(rp, rowptr) and np.array_equal(ad, adj) and np.array_equal(cnt, np.ones(len(adj), dtype=np.int64))


def test_all_equal_labels_give_one_vertex():
    for name, (V, src, dst) in R.hand_cases().items():
        rowptr, adj, _, _ = R.build(V, src, dst)
        rp, ad, cnt = R.quotient_dir(rowptr, adj, np.full(V, 9))
        assert rp.tolist() == [0, 1] and ad.tolist() == [0] and cnt.tolist() == [len(adj)], name
        rp, ad, cnt = R.quotient_dir(rowptr, adj, np.full(V, 9), drop_loops=True)
        assert rp.tolist() == [0, 0] and len(ad) == 0 and len(cnt) == 0, name


def test_composition_law():
    rng = np.random.default_rng(11)
    for trial in range(20):
        V = int(rng.integers(2, 65))
        src, dst = R.random_multigraph(rng, V, int(rng.integers(1, 5 * V)))
        rowptr, adj, _, _ = R.build(V, src, dst)
        a = rng.integers(0, max(V // 2, 1), size=V) * 5               # labels of the vertices
        cluster_of, label_of = R.vertex_maps(a)[:2]
        b = rng.integers(0, max(len(label_of) // 2, 1), size=len(label_of)) + 100      # labels of the coarse vertices
        w = rng.integers(1, 1 << 20, size=len(adj))
        for weights in (None, w):
            for drop in (False, True):
                first = R.quotient_dir(rowptr, adj, a, weights)
                twice = R.quotient_dir(first[0], first[1], b, first[2], drop)
                once = R.quotient_dir(rowptr, adj, b[cluster_of], weights, drop)
                assert same(twice, once), trial


def test_stats_and_their_bounds():
    V, src, dst = R.hand_cases()["star"]
    rowptr, adj, in_rowptr, in_adj = R.build(V, src, dst)
    labels = np.array([0, 1, 1, 1, 2, 2, 9])
    e_out, e_in = len(R.quotient_dir(rowptr, adj, labels)[1]), len(R.quotient_dir(in_rowptr, in_adj, labels)[1])
    st = R.quotient_stats(rowptr, in_rowptr, labels, e_out, e_in, short=1, wave=2, table=3)
    assert R.volumes(rowptr, labels).tolist() == [6, 3, 2, 1]
    assert (st["rows_short_out"], st["rows_wave_out"], st["rows_table_out"], st["rows_sorted_out"]) == (1, 1, 1, 1)
    assert st["sorted_keys_out"] == 6 and st["sort_pieces_out"] == 1 and st["entries_read_out"] == 12 and st["vertices"] == 4
    out_only = R.quotient_stats(rowptr, None, labels, e_out, 0)
    assert all(v == 0 for k, v in out_only.items() if k.endswith("_in")) and out_only["rows_short_out"] == 4
    assert R.class_rows([0, 0, 5]) == [1, 0, 0, 0]                     # rows of volume 0 are no items
    cap_keys = (1 << 20) // R.KEY_BYTES
    assert R.sort_pieces([cap_keys, 3, cap_keys + 5, 3, 3], table=2, cap_mb=1) == 4      # {cap}, {3}, {cap + 5} alone, {3, 3}
    assert R.sort_pieces([cap_keys, 3, cap_keys + 5, 3, 3], table=2, cap_mb=0) == 1
