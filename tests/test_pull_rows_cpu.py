"""The inputs of the pull-sum tests (tests/pull_rows_graphs.py) reach the paths of vgl_pull.h they are meant for, and tell a wrong sum from the
right one: every property is asserted here with numpy on the CSR the oracle builds, before any GPU is involved.

Paths and what pins them: ordinary rows (one thread per row, 2048-entry tiles, the 8-wide unroll and its remainder loop, the split of a 256-row
group into parts); hub wavefronts (rows of 512 and more, 512-value batches); giant workgroups (rounds of three batches, two slot sets); the unordered
chunk path of HITS (4096-entry chunks, the finish kernel).
"""
import numpy as np
import pytest

import pull_rows_graphs as P


@pytest.fixture(scope="module")
def oracle_csr(oracle):
    V, src, dst, rows = P.ladder()
    rowptr, adj, _ = oracle.coo_to_csr(V, src, dst)
    in_rowptr, in_adj = oracle.transpose_csr(rowptr, adj)
    return V, src, dst, rows, (rowptr, adj.astype(np.int64)), (in_rowptr, in_adj.astype(np.int64))


def _row(csr, v):
    return csr[1][csr[0][v]:csr[0][v + 1]]


def _loops(csr, v):
    return np.flatnonzero(_row(csr, v) == v).tolist()


def test_sizes_and_input_order(oracle_csr):
    V, src, dst, rows, out, _ = oracle_csr
    assert V == P.LADDER_V and 90_000 <= V <= 110_000 and V % P.BLOCK == 3
    assert src.dtype == np.int32 and dst.dtype == np.int32 and src.size == dst.size < 1_000_000
    assert src.min() >= 0 and dst.min() >= 0 and src.max() < V and dst.max() < V
    assert (np.diff(src.astype(np.int64)) < 0).sum() > 10_000                       # far from CSR order: all first entries, all second entries, ...
    # the order within a row is the input order: the oracle's stable build equals a stable sort by source
    order = np.argsort(src, kind="stable")
    assert (out[1] == dst[order]).all()
    assert int((src == dst).sum()) >= 800                                         # many self loops (the in-degree kernels take them off)


def test_long_rows(oracle_csr):
    V, _, _, rows, out, _ = oracle_csr
    deg = np.diff(out[0])
    for n in P.LONG_LENGTHS:
        plain, looped = int(rows["len%d" % n][0]), int(rows["len%d_loops" % n][0])
        assert deg[plain] == n and deg[looped] == n
        assert _loops(out, plain) == [] and _loops(out, looped) == P.loop_positions(n)
        for v in (plain, looped):
            e = _row(out, v)
            others = e[e != v]
            assert np.unique(others).size == others.size and (others >= P.PEERS[0]).all() and (others < sum(P.LIGHT)).all()
            assert (e[:513][e[:513] != v] < sum(P.PEERS)).all() and (e[513:][e[513:] != v] >= P.LIGHT[0]).all()
    assert [p for p in P.loop_positions(513)] == [0, 511, 512] and P.loop_positions(511) == [0, 510] and P.loop_positions(4097) == [0, 511, 512, 4096]
    v = int(rows["all_loops_600"][0])
    assert deg[v] == 600 and (_row(out, v) == v).all()
    v = int(rows["one_loop_512"][0])
    assert deg[v] == 512 == P.HUB_DEGREE and len(_loops(out, v)) == 1               # a hub by stored length, 511 entries summed
    assert deg[rows["extra_513_582"]].tolist() == list(range(513, 583))
    giants = {n: int(rows["giant_%d" % n][0]) for n in P.GIANT_LENGTHS}
    assert all(deg[v] == n for n, v in giants.items())
    assert [P.batches_and_rounds(n)[0] for n in P.GIANT_LENGTHS] == [64, 64, 65, 66]
    assert _loops(out, giants[32769]) == [0, 511, 512, 32768]
    # the rounds of the default giants come in both parities (the slot sets swap on k & 1; the last round ends in either set)
    default_giants = deg[deg >= P.GIANT_DEGREE]
    assert sorted(default_giants.tolist()) == [32768, 32769, 33281, P.TAIL_HUB]
    assert {P.batches_and_rounds(int(n))[1] % 2 for n in default_giants} == {0, 1}
    assert {P.batches_and_rounds(int(n))[0] % P.NP for n in default_giants} == {0, 1, 2}     # the last round holds 1, 2 and 3 batches


def test_ordinary_rows(oracle_csr):
    V, _, _, rows, out, _ = oracle_csr
    rowptr = out[0]
    deg = np.diff(rowptr)
    blk, parts = P.block_rows(rowptr)
    group = lambda first: first // P.BLOCK
    assert (deg[rows["group_511"]] == 511).all() and rows["group_511"].size == P.BLOCK and parts[group(P.G_511)] == 8
    assert rowptr[P.G_16384 + P.BLOCK] - rowptr[P.G_16384] == P.BLOCK_EDGES and parts[group(P.G_16384)] == 1
    assert rowptr[P.G_16385 + P.BLOCK] - rowptr[P.G_16385] == P.BLOCK_EDGES + 1 and parts[group(P.G_16385)] == 2
    # a row across the first tile boundary of its block and an empty row exactly on the second
    assert parts[group(P.G_STRADDLE)] == 1 and P.G_STRADDLE in blk
    e0 = rowptr[P.G_STRADDLE]
    v = int(rows["straddle"][0])
    assert (rowptr[v] - e0, rowptr[v + 1] - e0) == (P.TILE - 1, P.TILE + 1)
    v = int(rows["empty_at_tile"][0])
    assert rowptr[v] - e0 == 2 * P.TILE == rowptr[v + 1] - e0 and deg[v + 1] == 5
    assert (deg[rows["group_straddle"]] < P.HUB_DEGREE).all()
    # every length 1 .. 17 with its self loop in every position: each slot of the 8-wide unroll and of the remainder loop, at 0, 1 and 2 trips
    seen = sorted((int(deg[v]), _loops(out, v)[0]) for v in rows["unroll"] if len(_loops(out, v)) == 1)
    assert seen == [(n, p) for n in range(1, P.UNROLL_MAX + 1) for p in range(n)] and len(seen) == 153
    v = int(rows["adjacent_loops"][0])
    assert _loops(out, v) == [4, 5] and deg[v] == 10
    assert {1, 2, 8}.issubset(set(parts.tolist()))


def test_hub_placement(oracle_csr):
    V, _, _, rows, out, _ = oracle_csr
    rowptr = out[0]
    deg = np.diff(rowptr)
    blk, parts = P.block_rows(rowptr)
    assert parts[P.G_PLACE // P.BLOCK] == 1
    first, last, mid = int(rows["hub_first"][0]), int(rows["hub_last"][0]), int(rows["hub_mid_tile"][0])
    assert first == P.G_PLACE and first in blk and deg[first] >= P.HUB_DEGREE and _loops(out, first) == [0, 599]
    assert last == P.G_PLACE + P.BLOCK - 1 and last + 1 in blk and deg[last] == 513 and _loops(out, last) == [512]
    e0 = rowptr[P.G_PLACE]
    assert deg[mid] >= P.HUB_DEGREE and 0 < deg[mid - 1] < P.HUB_DEGREE and 0 < deg[mid + 1] < P.HUB_DEGREE
    # the first tile is skipped from the opening hub's end on, so the tiles of this block start at deg[first] + 2048 k: the hub begins inside one
    assert (rowptr[mid] - e0 - deg[first]) % P.TILE not in (0,) and (rowptr[mid] - e0 - deg[first]) // P.TILE == (rowptr[mid + 1] - 1 - e0 - deg[first]) // P.TILE
    a, b = (int(x) for x in rows["hubs_adjacent"])
    assert b == a + 1 and deg[a] >= P.HUB_DEGREE and deg[b] >= P.HUB_DEGREE
    # the final partial group: 3 rows, 40000+ entries; two rows per part are required, so the split stops at 2 parts
    tail = rows["tail_group"]
    assert tail.tolist() == [V - 3, V - 2, V - 1] and deg[V - 2] == P.TAIL_HUB and deg[V - 3] < P.HUB_DEGREE and deg[V - 1] < P.HUB_DEGREE
    e = rowptr[V] - rowptr[V - 3]
    assert e > 2 * P.BLOCK_EDGES and parts[-1] == 2 and blk[-3:].tolist() == [V - 3, V - 1, V]
    assert _loops(out, V - 2) == [0, 511, 512, P.TAIL_HUB - 1]
    assert {1, 2, 8}.issubset(set(parts.tolist())) and (parts <= 32).all()
    # shards: the middle one starts on the opening hub and owns the long rows with self loops
    lo, hi = P.SHARD_BOUNDS[1], P.SHARD_BOUNDS[2]
    assert lo == first and lo > 0 and all(lo <= int(rows["len%d_loops" % n][0]) < hi for n in P.LONG_LENGTHS)
    sblk, _ = P.block_rows(rowptr[lo:hi + 1] - rowptr[lo])
    assert sblk[0] == 0 and deg[lo + sblk[0]] >= P.HUB_DEGREE


def test_hub_and_giant_counts(oracle_csr):
    V, _, _, rows, out, inn = oracle_csr
    named = P.chain_rows(rows)
    deg = np.diff(out[0])
    assert sorted(np.flatnonzero(deg >= P.HUB_DEGREE).tolist()) == sorted(v for v in named.tolist() if deg[v] >= P.HUB_DEGREE)
    hubs, giants, chunks = P.hub_counts(out[0])
    assert hubs == 2 * len(P.LONG_LENGTHS) - 2 + 2 + 70 + 4 + 5 + 1 and giants == 4
    assert hubs > 4 * P.WAVES                                                     # VGL_PULL_HUB_BLOCKS=1: four wavefronts, several hubs each
    assert P.hub_counts(out[0], 513)[1] > P.GIANT_BLOCKS                          # some giant workgroup owns two rows or more
    forced = deg[(deg >= 513)]
    assert {2, 3, 4, 5, 6, 7}.issubset({P.batches_and_rounds(int(n))[0] for n in forced})
    assert 0 < P.hub_counts(out[0], 1025)[1] < P.hub_counts(out[0], 513)[1]
    assert int((deg >= P.CHUNK).sum()) >= 4 and chunks % 4 != 0                   # the out-direction has multi-chunk rows too (HITS' second half step)
    # in-direction: the ladder's targets and nothing else
    ideg = np.diff(inn[0])
    for n in P.IN_LENGTHS:
        assert ideg[int(rows["in_len%d" % n][0])] == n
    assert (ideg[rows["in_extra_512"]] == 512).all()
    ihubs, _, ichunks = P.hub_counts(inn[0])
    loops600 = int(rows["all_loops_600"][0])                                      # 600 self loops: an in-row of 600 entries as well
    assert sorted(np.flatnonzero(ideg >= P.HUB_DEGREE).tolist()) == sorted([loops600] + [int(v) for k, ids in rows.items() if k.startswith("in_") for v in ids])
    assert ihubs == len(P.IN_LENGTHS) + P.IN_EXTRA + 1 > P.BLOCK                  # the finish kernel runs two workgroups
    assert ichunks == 16 + P.IN_EXTRA + 1 and ichunks % 4 != 0                    # the last chunk workgroup has idle wavefronts


@pytest.fixture(scope="module")
def crafted(oracle_csr):
    V, _, _, rows, out, _ = oracle_csr
    indeg = P.crafted_indeg(V, P.under_test(rows))
    return indeg, P.first_contrib(V, indeg)


def test_crafted_in_degrees(oracle_csr, crafted):
    V, _, _, rows, out, _ = oracle_csr
    indeg, contrib = crafted
    assert indeg.dtype == np.int32 and indeg.min() == 0 and indeg.max() == 1 << 20
    peers = indeg[P.PEERS[0]:sum(P.PEERS)]
    assert 0.05 < (peers == 0).mean() < 0.08                                      # about one in 16
    for v in P.chain_rows(rows):
        e = _row(out, int(v))
        vals = indeg[e[e != v]]
        if vals.size >= 21:                                                       # (a doubled stretch starts at 3, not at 1)
            binades = np.unique(np.floor(np.log2(vals[vals > 0])).astype(int))
            assert binades.min() <= 1 and binades.max() >= 19 and binades.size >= 20 and (vals == 0).any()


def test_wrong_sums_differ_in_bits(oracle_csr, crafted):
    """the f32 adjacency-order chain of iteration 1 against: the order reversed, the last entry dropped, the entries past the last whole batch
    dropped, the self loops summed, entries 511 and 512 swapped.  A variant that sums the very same sequence (it drops or swaps self loops only, or
    reverses fewer than three terms: a + b == b + a) cannot differ and is counted, not asserted; such rows have a self-loop-free twin that does."""
    V, _, _, rows, out, _ = oracle_csr
    _, contrib = crafted
    same = {}
    checked = 0
    for v in np.concatenate([P.chain_rows(rows), rows["unroll"], rows["adjacent_loops"]]):
        e = _row(out, int(v))
        if e.size < 3:
            continue
        res = P.discriminates(int(v), e, contrib)
        assert "reversed" in res and "last_dropped" in res
        assert ("tail_dropped" in res and "swapped_511_512" in res) == (e.size > P.HUB_BATCH)
        assert ("self_included" in res) == bool((e == v).any())
        for name, r in res.items():
            assert r is not False, (name, int(v), e.size, P.case_of(rows, v))
            if r is None:
                same.setdefault(name, []).append(int(v))
            checked += r is True
    assert checked > 600
    # where nothing could differ: only rows with self loops or whole batches, or rows that sum fewer than three terms
    deg = np.diff(out[0])
    for name, vs in same.items():
        for v in vs:
            e = _row(out, v)
            assert (e == v).any() or (name == "tail_dropped" and e.size % P.HUB_BATCH == 0), (name, v)
    # the self-loop-free copy of every long length tells all four positional variants apart (whole batches: no tail to drop)
    for n in P.LONG_LENGTHS:
        res = P.discriminates(int(rows["len%d" % n][0]), _row(out, int(rows["len%d" % n][0])), contrib)
        assert all(r is True for k, r in res.items() if not (k == "tail_dropped" and n % P.HUB_BATCH == 0)), (n, res)
        assert res.get("self_included") is None
        assert P.discriminates(int(rows["len%d_loops" % n][0]), _row(out, int(rows["len%d_loops" % n][0])), contrib)["self_included"] is True


def test_oracle_chain_is_the_numpy_chain(oracle, oracle_csr, crafted):
    V, _, _, rows, out, _ = oracle_csr
    indeg, contrib = crafted
    got = oracle.pagerank(out[0], out[1].astype(np.int32), 1, 1, indeg=indeg)
    d = np.float32(0.85)
    k = np.float32((1.0 - np.float64(d)) / np.float64(np.float32(V)))
    dangling = np.float32(np.sum((np.full(V, np.float32(1.0 / V))[indeg == 0] / np.float32(V)).astype(np.float64)))
    for v in np.concatenate([P.chain_rows(rows), rows["unroll"], rows["adjacent_loops"], rows["tail_group"]]):
        terms = P.summed(int(v), _row(out, int(v)), contrib)
        acc = P.chain_f32(terms)
        assert np.float32(k + d * np.float32(acc + dangling)).view(np.int32) == got[v].view(np.int32), (int(v), P.case_of(rows, v))
        # n sequential roundings of at most 2^-24 relative each, all terms non-negative
        exact = float(np.sum(terms.astype(np.float64)))
        assert abs(float(acc) - exact) <= max(terms.size, 1) * 2.0 ** -24 * exact


def test_hits_chunk_order_margin(oracle, oracle_csr):
    """the chunk order of the unordered path, restated in numpy, stays within 1e-13 relative of the sequential chains of oracle.hits on these
    inputs: a tenfold margin under the 1e-12 the GPU test asserts"""
    V, _, _, rows, out, inn = oracle_csr
    wa, wh = oracle.hits(out[0], out[1].astype(np.int32), 2)
    a, h = P.hits_unordered(out, inn, 2)
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)))
    assert rel(a, wa) <= 1e-13 and rel(h, wh) <= 1e-13, (rel(a, wa), rel(h, wh))
    assert (wa[rows["in_len12289"]] > 0).all() and (wh[rows["giant_33281"]] > 0).all()
    # the restatement is not the sequential order: on the long rows the bits differ somewhere (otherwise this test would prove nothing)
    assert (a != wa).any() or (h != wh).any()


def test_small_graphs(oracle):
    V, src, dst = P.single_vertex_hub()
    assert V == 1 and src.size == 600 and (src == 0).all() and (dst == 0).all()
    V, src, dst = P.two_vertices()
    rowptr, adj, _ = oracle.coo_to_csr(V, src, dst)
    assert V == 2 and np.diff(rowptr).tolist() == [513, 0] and (adj == 1).all()
    V, src, dst = P.one_hub()
    rowptr, adj, _ = oracle.coo_to_csr(V, src, dst)
    hubs, giants, _ = P.hub_counts(rowptr)
    assert (hubs, giants) == (1, 0) and -(-hubs // P.WAVES) == 1                   # one hub workgroup: wavefronts 1 .. 3 own nothing
    assert np.flatnonzero(adj[rowptr[7]:rowptr[8]] == 7).tolist() == [0, 511, 512, 699]
