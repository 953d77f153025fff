"""The restatement of the subgraph contract (tests/subgraph_reference.py) against a brute force over the edge list and against closed forms, and the
library's new entry points.  No GPU: what the GPU tests compare the HIP path with is checked here first."""
import ctypes
import itertools

import numpy as np
import pytest

import subgraph_reference as R

CASES = R.hand_cases()


def masks_of(V, rng):
    yield None
    yield np.ones(V, dtype=np.uint8)
    yield (np.arange(V) % 2 == 0).astype(np.uint8)
    yield (np.arange(V) % 2 == 1).astype(np.uint8)
    for v in range(V):
        one = np.zeros(V, dtype=np.uint8)
        one[v] = 1
        yield one
    for _ in range(4):
        yield (rng.random(V) < 0.6).astype(np.uint8)


@pytest.mark.parametrize("name", sorted(CASES))
def test_filter_against_brute_force(name):
    V, src, dst = CASES[name]
    rowptr, adj, in_rowptr, in_adj = R.build(V, src, dst)
    rng = np.random.default_rng(7)
    for keep in masks_of(V, rng):
        for entry in (None, (rng.random(len(adj)) < 0.5).astype(np.uint8)):
            if keep is None and entry is None:
                continue
            vk, b_rp, b_adj, b_irp, b_iadj, b_org = R.filter_brute(V, rowptr, adj, keep, entry)
            rp, ad, org, new_id, old_id = R.filter_rows(rowptr, adj, keep, entry)
            assert len(old_id) == vk and np.array_equal(rp, b_rp) and np.array_equal(ad, b_adj) and np.array_equal(org, b_org)
            assert np.array_equal(new_id[old_id], np.arange(vk)) and int((new_id >= 0).sum()) == vk
            assert np.array_equal(adj[org], old_id[ad])               # the origin map
            if entry is None:                                         # a vertex mask alone: the incoming rows filter to from_coo's incoming CSR
                irp, iad, _, _, _ = R.filter_rows(in_rowptr, in_adj, keep)
                assert np.array_equal(irp, b_irp) and np.array_equal(iad, b_iadj)
            else:                                                     # an entry mask: the caller transposes
                irp, iad = R.transpose(vk, rp, ad)
                assert np.array_equal(irp, b_irp) and np.array_equal(iad, b_iadj)
            st = R.filter_stats(rowptr, adj, in_rowptr, in_adj, keep, entry)
            assert st["vertices_kept"] == vk and st["entries_kept_out"] == len(b_adj)
            assert st["entries_kept_in"] == (len(b_iadj) if entry is None else 0)
            assert st["rows_short_out"] + st["rows_wave_out"] + st["rows_wg_out"] == vk


def test_closed_forms():
    V, src, dst = CASES["star"]
    rowptr, adj, in_rowptr, in_adj = R.build(V, src, dst)
    keep = np.ones(V, dtype=np.uint8)
    keep[0] = 0                                                       # the hub dropped: no edge is left
    rp, ad, _, _, old = R.filter_rows(rowptr, adj, keep)
    assert len(ad) == 0 and rp.tolist() == [0] * V and old.tolist() == list(range(1, V))
    for n, m in ((5, 3), (9, 4), (6, 6), (7, 1)):                     # K_n with m vertices kept is K_m
        s, d = R._both([(i, j) for i in range(n) for j in range(i + 1, n)])
        rowptr, adj, _, _ = R.build(n, s, d)
        keep = np.zeros(n, dtype=np.uint8)
        keep[np.random.default_rng(n).permutation(n)[:m]] = 1
        rp, ad, _, _, _ = R.filter_rows(rowptr, adj, keep)
        assert np.diff(rp).tolist() == [m - 1] * m
        assert [sorted(ad[rp[i]:rp[i + 1]].tolist()) for i in range(m)] == [[j for j in range(m) if j != i] for i in range(m)]
    for name in CASES:                                                # everything kept: the identity
        V, src, dst = CASES[name]
        rowptr, adj, in_rowptr, in_adj = R.build(V, src, dst)
        rp, ad, org, new_id, old_id = R.filter_rows(rowptr, adj, np.ones(V, dtype=np.uint8))
        assert np.array_equal(rp, rowptr) and np.array_equal(ad, adj) and np.array_equal(org, np.arange(len(adj))) and np.array_equal(new_id, np.arange(V))
        st = R.filter_stats(rowptr, adj, in_rowptr, in_adj, np.ones(V, dtype=np.uint8))
        assert st["entries_read_out"] == st["entries_kept_out"] == st["entries_read_in"] == st["entries_kept_in"] == len(adj)
        assert st["algorithmic_bytes"] == V + 4 * V + 4 * V + 2 * (56 * V + 32 * (V + 1) + 20 * len(adj))


@pytest.mark.parametrize("name", sorted(CASES))
def test_k_hop_against_brute_force(name):
    V, src, dst = CASES[name]
    rowptr, adj, in_rowptr, in_adj = R.build(V, src, dst)
    for seeds, hops, (direction, symmetric) in itertools.product(([0], [V - 1, V - 1, 0], list(range(V)), []), (0, 1, 2, 10 ** 6),
                                                                  ((0, False), (1, False), (0, True))):
        hop, st = R.k_hop(rowptr, adj, in_rowptr, in_adj, seeds, hops, direction, symmetric)
        assert np.array_equal(hop, R.k_hop_brute(V, src, dst, seeds, hops, direction, symmetric)), (seeds, hops, direction, symmetric)
        assert st["reached"] == int((hop >= 0).sum()) and st["levels_run"] <= hops
        if hops == 0:
            assert sorted(np.nonzero(hop == 0)[0].tolist()) == sorted(set(seeds)) and st["levels_run"] == 0
    V, src, dst = CASES["path"]
    rowptr, adj, in_rowptr, in_adj = R.build(V, src, dst)
    assert R.k_hop(rowptr, adj, in_rowptr, in_adj, [0], 3)[0].tolist() == [0, 1, 2, 3, -1, -1]


def test_key_is_the_api_priority_key():
    torch = pytest.importorskip("torch")
    from vectorgraphlibrary_amd import api
    ids = np.array([0, 1, 2, 12345, 2 ** 31, 2 ** 32 - 1], dtype=np.int64)
    for seed in (0, 1, 0xFFFFFFFF):
        assert R.key(ids, seed).tolist() == api.priority_key(torch.tensor(ids), seed).tolist()


@pytest.mark.parametrize("name", sorted(CASES))
def test_selection_against_brute_force(name):
    V, src, dst = CASES[name]
    rowptr, adj, in_rowptr, in_adj = R.build(V, src, dst)
    seeds = list(range(V)) + [0, 0]
    for fanout, seed, (rp_, ad_) in itertools.product((1, 2, 3, 100), (0, 9), ((rowptr, adj), (in_rowptr, in_adj))):
        rp, ad, org, st = R.sample(rp_, ad_, seeds, fanout, seed)
        want = R.sample_brute(rp_, ad_, seeds, fanout, seed)
        for i in range(len(seeds)):
            assert list(zip(org[rp[i]:rp[i + 1]].tolist(), ad[rp[i]:rp[i + 1]].tolist())) == want[i]
        deg = np.diff(rp_)[seeds]
        assert np.diff(rp).tolist() == np.minimum(deg, fanout).tolist()
        assert st["sampled_total"] == len(ad) and st["entries_examined"] == int(deg.sum()) and st["rows_short"] == len(seeds)
        assert st["algorithmic_bytes"] == 60 * len(seeds) + 16 * (len(seeds) + 1) + 8 * len(ad)


def test_sample_blocks_structure():
    V, src, dst = CASES["k5"]
    rowptr, adj, _, _ = R.build(V, src, dst)
    blocks = R.sample_blocks(rowptr, adj, [3, 3, 1], [2, 1, 4], 5)
    assert len(blocks) == 3 and blocks[0][0].tolist() == [3, 3, 1]
    for h, (front, rp, ad) in enumerate(blocks):
        assert len(rp) == len(front) + 1 and rp[-1] == len(ad)
        want_rp, want_ad, _, _ = R.sample(rowptr, adj, front, [2, 1, 4][h], 5 + h)
        assert np.array_equal(rp, want_rp) and np.array_equal(ad, want_ad)
        if h + 1 < len(blocks):
            nxt = blocks[h + 1][0]
            assert nxt.tolist() == sorted(set(front.tolist()) | set(ad.tolist()))
    assert np.array_equal(blocks[0][1][:2], [0, 2]) and blocks[0][2][:2].tolist() == blocks[0][2][2:4].tolist()      # a repeated seed: a row of its own, the same row


NEW_ENTRIES = ("vgl_hip_subgraph_plan_create", "vgl_hip_subgraph_plan_info", "vgl_hip_subgraph_plan_vertex_maps", "vgl_hip_subgraph_plan_fill",
               "vgl_hip_subgraph_plan_destroy", "vgl_hip_khop_run", "vgl_hip_sample_neighbors")


def test_library_exports_and_binds_the_new_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from vectorgraphlibrary_amd import api, lib
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(L, name), name + " is not exported"
        assert name in lib._SIGNATURES, name + " is not bound"
    for cls, fields in ((lib.SubgraphStats, 12), (lib.KhopStats, 4), (lib.SampleStats, 7)):
        assert len(cls._fields_) == fields
    assert ctypes.sizeof(lib.SubgraphStats) == 96 and ctypes.sizeof(lib.KhopStats) == 32 and ctypes.sizeof(lib.SampleStats) == 56
    for fn in ("induced_subgraph", "edge_subgraph", "k_hop", "ego_graph", "sample_neighbors", "sample_blocks"):
        assert callable(getattr(api, fn))
    bound = lib.load()
    plan = ctypes.c_void_p()                                          # every entry refuses a NULL context before it touches anything
    assert bound.vgl_hip_subgraph_plan_create(None, None, None, None, ctypes.byref(plan)) != 0 and plan.value is None
    assert b"subgraph_plan_create" in bound.vgl_hip_last_error()
    assert bound.vgl_hip_khop_run(None, None, None, 0, 1, 0, 0, None, None) != 0 and b"khop_run" in bound.vgl_hip_last_error()
    assert bound.vgl_hip_sample_neighbors(None, None, None, 0, 1, 0, 0, None, None, None, None) != 0 and b"sample_neighbors" in bound.vgl_hip_last_error()
    assert bound.vgl_hip_subgraph_plan_fill(None, None, 0, None, None, None) != 0
