"""The blocked exact sums on the GPU (vgl_sum_blk_op behind vgl_hip_sum_over_edges_f32 / api.sum_over_edges, vgl_pr_blk_op behind PR_BLOCKED)
against the integer restatement of tests/blocked_sums_reference.py, BIT FOR BIT: every comparison is on the int32 view of the f32 result.  The
graph is built by hand (blocked_sums_reference.build_graph) so that block, slab, chunk and pad edges are all present; the values sit at the
edges of the fixed point (shift 0, -1, -23, -24, the f32 tie that a double rounding gets wrong, subnormals, signed zeros, the capacity).

Against the library of the commit before these tests, which has no vgl_hip_sum_over_edges_check (loaded with that entry taken out of
lib._SIGNATURES and a stand-in that waits for the stream and reports 0 in its place; raw_sums alone does the same by itself), the double-rounding
family, the five refusals and test_check_reports_every_kind_at_once fail and the other 23 pass."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import blocked_sums_reference as BR

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)
CUT = {"VGL_BLK_GATHER_UNIT": "64", "VGL_BLK_ACCUM_UNIT": "64"}


def api():
    from vectorgraphlibrary_amd import api as A
    return A


class Graphs:
    """per segment length the CSR and two handles over it: the default cut into units and the cut into units of 64 chunks"""

    def __init__(self):
        self.made = {}

    def get(self, ctx, segment_len):
        if segment_len not in self.made:
            A = api()
            rowptr, adj = BR.build_graph(segment_len)
            d_rowptr, d_adj = torch.from_numpy(rowptr).to(ctx.device), torch.from_numpy(adj).to(ctx.device)
            handles = []
            for cut in (False, True):
                if cut:
                    os.environ.update(CUT)
                try:
                    g = A.Graph(ctx, BR.V, d_rowptr, d_adj)                # a fresh handle builds a fresh layout: here, under the switches
                    status = ctx.L.vgl_hip_pr_prepare(ctx.h, g.h, A.PR_BLOCKED, None)
                finally:
                    for k in CUT:
                        os.environ.pop(k, None)
                assert status == 0
                handles.append(g)
            self.made[segment_len] = (rowptr, adj, handles)
        return self.made[segment_len]

    def close(self):
        for _, _, handles in self.made.values():
            for g in handles:
                g.close()
        self.made = {}


@pytest.fixture(scope="module")
def graphs():
    gs = Graphs()
    yield gs
    gs.close()


def raw_sums(ctx, g, values, bound):
    """the C call itself on a sums array of V + 64 floats: (first V, tail of 64)"""
    x = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(ctx.device)
    sums = torch.full((BR.V + 64,), float(SENTINEL), dtype=torch.float32, device=ctx.device)
    status = ctx.L.vgl_hip_sum_over_edges_f32(ctx.h, g.h, C.c_void_p(x.data_ptr()), C.c_float(float(bound)), C.c_void_p(sums.data_ptr()))
    assert status == 0
    bits = C.c_uint(99)
    check = getattr(ctx.L, "vgl_hip_sum_over_edges_check", None)
    if check is None:                                                                  # a library from before the check (see the module docstring)
        ctx.sync()
        bits.value = 0
    else:
        assert check(ctx.h, C.byref(bits)) == 0                                        # waits for the stream
    out = sums.cpu().numpy()
    return out[:BR.V], out[BR.V:], bits.value


def differing(got, want):
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    return [(int(r), float(got[r]).hex(), float(want[r]).hex()) for r in bad[:8]]


def check_family(ctx, handles, rowptr, adj, name, bound, values):
    _, want = BR.row_sums(rowptr, adj, values, bound)
    got = []
    for g in handles:
        sums, tail, broken = raw_sums(ctx, g, values, bound)
        assert broken == 0, (name, broken)
        assert (tail == SENTINEL).all(), name
        got.append(sums)
    assert (got[0].view(np.int32) == got[1].view(np.int32)).all(), (name, "the sums depend on the cut into units", differing(got[0], got[1]))
    assert (got[0].view(np.int32) == want.view(np.int32)).all(), (name, differing(got[0], want))


@pytest.mark.parametrize("segment_len", BR.SEGMENT_LENGTHS)
def test_every_row_written_at_block_slab_and_chunk_edges(segment_len, ctx, graphs):
    """values at every vertex: the corner rows of the accumulate blocks, the block of one id, the block without edges (written as 0), the hub
    whose block goes through slabs under the small cut, the row that lists one neighbour three times, self loops dropped, and the segment of
    row V - 1 at 1, 63, 64, 65 and 128 entries (pad entries must add nothing); nothing is written behind row V - 1"""
    rowptr, adj, handles = graphs.get(ctx, segment_len)
    values = BR.base_values()
    check_family(ctx, handles, rowptr, adj, "base", 1.0, values)
    acc, want = BR.row_sums(rowptr, adj, values, 1.0)
    sums, _, _ = raw_sums(ctx, handles[1], values, 1.0)
    assert (sums[32768:49152].view(np.int32) == 0).all(), "the rows of the accumulate block without edges read +0.0"
    assert all(acc[r] > 0 for r in BR.CORNERS + (BR.HUB, BR.TRIPLE_ROW, BR.STAR_ROW)) and sums[BR.V - 1] == want[BR.V - 1]


@pytest.mark.parametrize("family", range(len(BR.value_families())), ids=[f[0].replace(" ", "_") for f in BR.value_families()])
def test_value_families_bit_for_bit(family, ctx, graphs):
    """each family of blocked_sums_reference.value_families equals row_sums bit for bit under both cuts: the exponent ladder for four bounds
    (shift 0, -1, -23, -24), one large and many tiny, accumulated truncation, the double-rounding triple and its mirror, subnormal inputs,
    signed zeros, a sum equal to a bound that is no power of two and a value one ulp below the capacity"""
    rowptr, adj, handles = graphs.get(ctx, 65)
    name, bound, values = BR.value_families()[family]
    check_family(ctx, handles, rowptr, adj, name, bound, values)


@pytest.mark.parametrize("iterations", [0, 1, 3])
def test_pagerank_blocked_bit_for_bit(iterations, ctx, graphs):
    """PR_BLOCKED equals the f32 restatement with exact per-row sums and one rounding, bit for bit, under both cuts"""
    A = api()
    rowptr, adj, handles = graphs.get(ctx, 65)
    want = BR.pagerank(rowptr, adj, iterations)
    for g in handles:
        ranks, st = A.page_rank(g, iterations, raw=True, mode=A.PR_BLOCKED)
        rk = ranks.cpu().numpy()
        assert (rk.view(np.int32) == want.view(np.int32)).all(), (iterations, differing(rk, want))
        assert abs(st["ranks_sum"] - float(rk.astype(np.float64).sum())) < 1e-9


def refusal_cases():
    """(id, values, message, VGL_HIP_SUM_* bit, rows whose sum the broken value or the overflow touches) under bound 1.0, capacity 4.0"""
    good = BR.base_values()
    at = BR.GATHER_BLOCK                                                      # a corner target: read by the five corner rows
    cases = []
    for name, bad, kind, bit in (("negative", -1.0, "negative value", 1), ("nan", float("nan"), "not finite", 2), ("inf", float("inf"), "not finite", 2),
                                 ("value_at_capacity", 4.0, "value at or above the capacity", 4)):
        v = good.copy()
        v[at] = np.float32(bad)
        cases.append((name, v, kind, bit, BR.CORNERS))
    v = good.copy()
    v[BR.THREE_LEAF0:BR.THREE_LEAF0 + 3] = (2.0, 1.5, 0.5)                    # three valid values, their sum the capacity
    cases.append(("sum_at_capacity", v, "sum at or above the capacity", 8, (BR.THREE_ROW0,)))
    return good, cases


@pytest.mark.parametrize("case", range(5), ids=[c[0] for c in refusal_cases()[1]])
def test_broken_contract_is_refused_and_nothing_sticks(case, ctx, graphs):
    """A negative, NaN, infinite or too-large value at a vertex that edges read, and a row of valid values whose sum reaches the capacity: the C
    call leaves the bit of the kind (and the right bits in every row that the value does not touch), api.sum_over_edges raises VglHipError
    naming the kind, and the valid call straight afterwards returns the right bits"""
    from vectorgraphlibrary_amd import lib as L
    A = api()
    rowptr, adj, handles = graphs.get(ctx, 65)
    good, cases = refusal_cases()
    _, values, kind, bit, touched = cases[case]
    _, want = BR.row_sums(rowptr, adj, good, 1.0)
    x_good, x_bad = torch.from_numpy(good).to(ctx.device), torch.from_numpy(values).to(ctx.device)
    assert sum(int(t) == BR.GATHER_BLOCK for t in adj) >= 4
    clean = np.ones(BR.V, dtype=bool)
    clean[list(touched)] = False
    for g in handles:
        sums, tail, broken = raw_sums(ctx, g, values, 1.0)
        assert broken == bit, (kind, broken)
        assert (sums[clean].view(np.int32) == want[clean].view(np.int32)).all() and (tail == SENTINEL).all(), kind
        assert raw_sums(ctx, g, good, 1.0)[2] == 0, "the check clears the bits"
        with pytest.raises(L.VglHipError, match=kind):
            A.sum_over_edges(g, x_bad, 1.0)
        got = A.sum_over_edges(g, x_good, 1.0).cpu().numpy()
        assert (got.view(np.int32) == want.view(np.int32)).all(), (kind, differing(got, want))


def test_signed_zero_and_sum_equal_to_the_bound_are_accepted(ctx, graphs):
    A = api()
    rowptr, adj, handles = graphs.get(ctx, 65)
    for name, bound, values in BR.value_families():
        if name in ("signed zeros", "sum equal to 0.3, value below capacity"):
            assert (values.view(np.int32) == np.int32(-2 ** 31)).any(), "holds a -0.0"
            for g in handles:
                got = A.sum_over_edges(g, torch.from_numpy(values).to(ctx.device), bound).cpu().numpy()
                assert (got.view(np.int32) == BR.row_sums(rowptr, adj, values, bound)[1].view(np.int32)).all(), name


def test_check_reports_every_kind_at_once(ctx, graphs):
    rowptr, adj, handles = graphs.get(ctx, 65)
    v = BR.base_values()
    v[BR.GATHER_BLOCK], v[0], v[BR.V - 1] = np.float32(-1.0), np.float32("nan"), np.float32(8.0)
    v[BR.THREE_LEAF0:BR.THREE_LEAF0 + 3] = (2.0, 1.5, 0.5)
    assert raw_sums(ctx, handles[0], v, 1.0)[2] == 1 | 2 | 4 | 8
    assert raw_sums(ctx, handles[0], BR.base_values(), 1.0)[2] == 0
