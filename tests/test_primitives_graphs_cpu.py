"""The inputs of the operator-primitive self-check reach the branches they are meant for: every property is asserted here with numpy on the
outgoing CSR and on the incoming CSR, computed the way the library computes it (tests/primitives_graphs.py), before any GPU is involved."""
import numpy as np
import pytest

import primitives_graphs as P


@pytest.fixture(scope="module")
def ragged():
    V, src, dst = P.ragged()
    return V, src, dst, {fmt: P.both_directions(V, src, dst, fmt) for fmt in ("csr", "vcsr")}


DIRECTIONS = [0, 1]


def test_ragged_sizes(ragged):
    V, src, dst, _ = ragged
    assert V == 1024 * 256 + 77 and V > P.REDUCE_GRID * P.BLOCK                  # a reduce workgroup folds more than one stride
    assert all(V % m for m in (8, 64, 256, 2048))
    assert src.dtype == np.int32 and dst.dtype == np.int32 and src.size == dst.size < 1_000_000
    assert src.min() >= 0 and dst.min() >= 0 and src.max() < V and dst.max() < V
    assert (src == dst).sum() >= 2                                                # self loops
    pairs = src.astype(np.int64) * V + dst
    assert np.unique(pairs).size < pairs.size                                     # duplicate edges
    # not in CSR order already
    assert (np.diff(src.astype(np.int64)) < 0).any()


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_ragged_rows(ragged, direction):
    V, _, _, built = ragged
    rowptr, adj = built["csr"][direction]
    deg = np.diff(rowptr)
    assert rowptr[-1] == adj.size
    assert (deg[:P.EMPTY_ENDS] == 0).all() and (deg[-P.EMPTY_ENDS:] == 0).all()   # empty rows at both ends
    first, count = P.STRETCH
    assert count >= 6000
    assert (deg[first:first + count] == np.asarray(P.STRETCH_DEGREES)[(np.arange(count) + direction * P.STRETCH_ROTATE) % 6]).all()
    assert (deg > 2 * P.TILE).sum() >= 2 and (deg > P.CHUNK).sum() >= 2            # two rows longer than two tiles / one chunk
    assert deg.max() > 2 * P.CHUNK                                                 # one of them spans more than two chunks
    starts = rowptr[:-1][deg > 0]
    assert ((starts % P.TILE == 0) & (starts > 0)).any()                           # a row that begins exactly on a tile boundary
    assert P.long_rows(rowptr) >= 2 and P.multi_chunk_blocks(rowptr) >= 2


def test_ragged_directions_differ(ragged):
    """a primitive that looks at the other direction's rows cannot pass: the degrees differ per vertex and summed over either partial frontier"""
    V, _, _, built = ragged
    out_deg, in_deg = np.diff(built["csr"][0][0]), np.diff(built["csr"][1][0])
    assert (out_deg != in_deg).sum() >= 60000
    for kind in ("sparse", "large"):
        ids = P.frontier_ids(V, kind)
        assert out_deg[ids].sum() != in_deg[ids].sum()
    assert out_deg[1000] != in_deg[1000] and min(out_deg[1000], in_deg[1000]) > P.CHUNK


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_ragged_wavefronts(ragged, direction):
    """rows of 1 .. 7 entries next to rows of 8 .. 63 inside one wavefront of a tile advance, wavefronts that sit inside one row (the combined add)
    and wavefronts with several rows (per-lane adds)"""
    V, _, _, built = ragged
    rowptr, _ = built["csr"][direction]
    deg = np.diff(rowptr)
    rows = np.repeat(np.arange(V), deg)
    wave = np.arange(rows.size) // P.WAVE
    small = np.zeros(wave[-1] + 1, bool)
    medium = np.zeros(wave[-1] + 1, bool)
    small[wave[(deg[rows] >= 1) & (deg[rows] <= 7)]] = True
    medium[wave[(deg[rows] >= 8) & (deg[rows] <= 63)]] = True
    assert (small & medium).sum() >= 100
    combined, mixed = P.wave_kinds(rowptr)
    assert combined >= 100 and mixed >= 100


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("kind", ["sparse", "large"])
def test_ragged_sparse_tiles_go_unstaged(ragged, direction, kind):
    """both partial frontiers have 2048-edge tiles that span more than 1024 frontier positions (CSR_GRAPH keeps both SPARSE), and tiles that do not"""
    V, _, _, built = ragged
    rowptr, _ = built["csr"][direction]
    spans = P.sparse_tile_spans(rowptr, P.frontier_ids(V, kind))
    assert (spans > P.STAGE).sum() >= 2 and (spans <= P.STAGE).sum() >= 2
    assert P.unstaged_tiles(rowptr, P.frontier_ids(V, kind)) == (spans > P.STAGE).sum()


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("fmt", ["csr", "vcsr"])
def test_ragged_coverage_facts_are_positive(ragged, fmt, direction):
    V, _, _, built = ragged
    rowptr, _ = built[fmt][direction]
    facts = P.coverage(rowptr, V)
    assert all(v > 0 for v in facts.values()), facts
    if fmt == "vcsr":                                                              # the large partial frontier is DENSE there
        assert (V - (V + 10) // 11) / V > 0.7


def test_tile_span_arithmetic():
    """sparse_tile_spans on cases small enough to do by hand"""
    rowptr = np.array([0, 0, 2048, 2048, 2049, 4097])                              # degrees 0, 2048, 0, 1, 2048
    ids = np.arange(5)
    # offsets 0 0 2048 2048 2049 4097: edge 0 belongs to position 1, edge 2048 to position 3, edge 4096 and the last edge to position 4
    assert P.sparse_tile_spans(rowptr, ids).tolist() == [3, 2, 1]
    ones = np.arange(0, 5001)                                                      # 5000 rows of one entry: owners 0, 2048, 4096, then 4999
    assert P.sparse_tile_spans(ones, np.arange(5000)).tolist() == [2049, 2049, 904]
    assert P.unstaged_tiles(ones, np.arange(5000)) == 2
    assert P.sparse_tile_spans(np.zeros(4, np.int64), np.arange(3)).size == 0


def test_small_graphs():
    V, src, dst = P.tiny()
    assert V == 1 and src.tolist() == [0] and dst.tolist() == [0]
    V, src, dst = P.no_edges()
    assert V == 5 and src.size == 0 and dst.size == 0
    V, src, dst = P.three_edges()
    assert V == 70 and src.size == 3 and V % 8 and V % 64
    for name, make in P.GRAPHS.items():
        V, src, dst = make()
        (orp, oadj), (irp, iadj) = P.both_directions(V, src, dst)
        assert orp[-1] == irp[-1] == src.size
        # the incoming CSR is the transpose
        out_pairs = sorted(zip(np.repeat(np.arange(V), np.diff(orp)).tolist(), oadj.tolist()))
        in_pairs = sorted(zip(iadj.tolist(), np.repeat(np.arange(V), np.diff(irp)).tolist()))
        assert out_pairs == in_pairs, name
