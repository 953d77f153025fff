"""The restatement of the blocked exact sums (tests/blocked_sums_reference.py) checked on its own, without a GPU: the fixed point against
fractions.Fraction, the single rounding against the double rounding it replaces, the exponent of the bound, and the conditions that the graph
and the value families of tests/test_blocked_sums_gpu.py have to meet for a bit-for-bit comparison."""
import math
from fractions import Fraction

import numpy as np
import pytest

import blocked_sums_reference as BR


def f32_fraction(bits):
    return Fraction(float(np.array([bits], dtype=np.uint32).view(np.float32)[0]))


def bits_of(mantissa, sh, bound_exp):
    """the bits of the normal f32 with this 24-bit mantissa whose shift is sh under bound_exp"""
    ex = sh + 150 - 62 + bound_exp
    assert 1 <= ex <= 254 and 0x800000 <= mantissa <= 0xFFFFFF
    return (ex << 23) | (mantissa & 0x7FFFFF)


@pytest.mark.parametrize("bound_exp", [0, 2, -1, 11, 62, -117])
def test_to_units_against_fractions(bound_exp):
    unit = Fraction(2) ** (bound_exp - 62)
    rng = np.random.default_rng(bound_exp + 200)
    for sh in range(-30, 39):
        for m in [0x800000, 0xFFFFFF, 0x800001, 0xAAAAAB] + rng.integers(0x800000, 0x1000000, 4).tolist():
            ex = sh + 150 - 62 + bound_exp
            if not 1 <= ex <= 254:
                continue
            bits = bits_of(m, sh, bound_exp)
            exact = f32_fraction(bits) / unit
            got = BR.to_units(bits, bound_exp)
            if sh >= 0:
                assert got == exact, (sh, hex(m))
            else:
                assert 0 <= exact - got < 1, (sh, hex(m))
                assert got == math.floor(exact), "a truncation, not a rounding"
            if sh <= -24:
                assert got == 0
            if sh == -23:
                assert got == 1                                           # both 0x800000 and 0xFFFFFF keep exactly their top bit
    for m in (0x800000, 0xFFFFFF):
        if 1 <= -24 + 88 + bound_exp <= 254:
            assert BR.to_units(bits_of(m, -24, bound_exp), bound_exp) == 0 and BR.to_units(bits_of(m, -23, bound_exp), bound_exp) != 0


def test_to_units_zeros_and_subnormals():
    assert BR.to_units(0x00000000, 2) == 0 and BR.to_units(0x80000000, 2) == 0          # +0.0 and -0.0
    be = BR.bound_exp_of(2.0 ** -119)
    assert be == -117
    big = int(BR.LARGEST_SUBNORMAL.view(np.uint32))
    assert big == 0x007FFFFF and BR.to_units(big, be) == 0x7FFFFF << 30                  # exponent field 0 is read as 1, no hidden bit
    assert BR.to_units(big, be) * Fraction(2) ** (be - 62) == f32_fraction(big)
    assert BR.to_units(0x00800000, be) == 0x800000 << 30                                 # the smallest normal continues the subnormals
    # PageRank's to_fixed is bound_exp = 0: 1.0 is 2^62 units, 2^-39 the smallest value whose whole mantissa converts
    assert BR.to_units(BR.f32_bits(1.0), 0) == 1 << 62
    assert BR.to_units(BR.f32_bits(np.float32(0xFFFFFF) * BR.pow2(-62)), 0) == 0xFFFFFF
    assert BR.to_units(BR.f32_bits(np.float32(0xFFFFFF) * BR.pow2(-63)), 0) == 0xFFFFFF >> 1


def test_bound_exp_of():
    assert BR.bound_exp_of(1.0) == 2                                                      # unit 2^-60
    assert BR.bound_exp_of(0.3) == 0
    assert BR.bound_exp_of(1000.0) == 11
    assert BR.bound_exp_of(2.0 ** 60) == 62
    assert BR.bound_exp_of(2.0 ** -119) == -117
    below = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    assert BR.bound_exp_of(below) == 1 and BR.bound_exp_of(float(np.nextafter(np.float32(1024.0), np.float32(0.0)))) == 11
    for b in (1.0, 0.3, 1000.0, 2.0 ** 60, 2.0 ** -119, below):
        be = BR.bound_exp_of(b)
        assert 2.0 ** (be - 2) <= float(np.float32(b)) < 2.0 ** (be - 1)                   # the capacity 2^be is above twice the bound


def test_round_once_against_fractions():
    rng = np.random.default_rng(3)
    cases = [(1 << 59) + (1 << 35) + 1, (1 << 59) + (1 << 35), (1 << 59) + (1 << 35) - 1, (1 << 59) + (1 << 36) + (1 << 35), (1 << 62) - 1,
             (1 << 24) + 1, (1 << 25) + 2, (1 << 25) + 6, 1, 0xFFFFFF, 0x1FFFFFF]
    cases += [int(x) for x in rng.integers(1, 1 << 62, 200)]
    for acc in cases:
        got = Fraction(float(BR.round_once(acc, -60)))
        exact = Fraction(acc, 1 << 60)
        lo = Fraction(float(np.nextafter(np.float32(float(got)), np.float32(0.0))))
        hi = Fraction(float(np.nextafter(np.float32(float(got)), np.float32(np.inf))))
        assert abs(got - exact) <= abs(lo - exact) and abs(got - exact) <= abs(hi - exact), "the nearest f32"
        if abs(got - exact) == abs(hi - exact) or abs(got - exact) == abs(lo - exact):    # a tie: the even mantissa
            assert int(np.float32(float(got)).view(np.uint32)) % 2 == 0
    with pytest.raises(AssertionError):
        BR.round_once(1, -140)                                                             # a subnormal result is outside the contract


def test_single_and_double_rounding_differ_on_the_triple_and_its_mirror():
    rowptr = np.array([0, 3, 6], dtype=np.int64)
    adj = np.array([2, 3, 4, 5, 6, 7], dtype=np.int32)
    values = np.zeros(8, dtype=np.float32)
    values[2:5], values[5:8] = BR.TRIPLE, BR.MIRROR
    assert [float(x) for x in values[2:8]] == list(BR.TRIPLE) + list(BR.MIRROR), "the six values are f32"
    rowptr = np.concatenate([rowptr, np.full(6, 6, dtype=np.int64)])
    acc, want = BR.row_sums(rowptr, adj, values, 1.0)
    assert acc[0] == (1 << 59) + (1 << 35) + 1 and acc[1] == (1 << 59) + (1 << 36) + (1 << 35) - 1
    assert float(want[0]) == 0.5 + 2.0 ** -24 and float(BR.double_rounded(acc[0], 2)) == 0.5
    assert float(want[1]) == 0.5 + 2.0 ** -24 and float(BR.double_rounded(acc[1], 2)) == 0.5 + 2.0 ** -23
    # the two conversions agree wherever 53 bits hold the accumulator
    for a in (1, (1 << 53) - 1, (1 << 59) + (1 << 35), (1 << 61) + (1 << 9)):
        assert BR.double_rounded(a, 2) == BR.round_once(a, -60)


def test_row_sums_skips_self_loops_and_counts_duplicates():
    rowptr = np.array([0, 4, 4, 6], dtype=np.int64)
    adj = np.array([0, 1, 1, 2, 2, 0], dtype=np.int32)
    values = np.array([0.5, 0.25, 0.125], dtype=np.float32)
    acc, want = BR.row_sums(rowptr, adj, values, 1.0)
    assert acc == [(2 << 58) + (1 << 57), 0, 1 << 59] and want.tolist() == [0.625, 0.0, 0.5]


@pytest.mark.parametrize("segment_len", BR.SEGMENT_LENGTHS)
def test_graph_has_the_edges_the_layout_must_handle(segment_len):
    rowptr, adj = BR.build_graph(segment_len)
    V = BR.V
    assert V == 49153 and len(rowptr) == V + 1 and len(adj) <= 30000
    assert (np.diff(rowptr)[32768:49152] == 0).all(), "accumulate block 2 has no edge"
    rows = np.repeat(np.arange(V), np.diff(rowptr))
    for r in BR.CORNERS:
        mine = adj[rows == r].tolist()
        assert all(t in mine for t in BR.CORNER_TARGETS) and r in mine
    last = adj[rows == V - 1]
    assert int(((last >= 32768) & (last != V - 1)).sum()) == segment_len               # the segment (gather block 1, accumulate block 3)
    hub = adj[rows == BR.HUB]
    assert len(hub) == 9000 and (hub < 32768).sum() > 64 * 64 and (hub >= 32768).sum() > 64 * 64 and len(set(hub.tolist())) == 9000
    kept = int((adj[rows < 16384] != rows[rows < 16384]).sum())
    assert kept / 64 > 2 * 64, "accumulate block 0 is cut into at least three units of at most 64 chunks"
    assert (adj[rows == BR.TRIPLE_ROW] == BR.HUB).sum() == 3


def test_pagerank_condition_holds_on_the_test_graphs():
    for segment_len in BR.SEGMENT_LENGTHS:                                                # every graph of the GPU tests (PageRank runs on 65)
        rowptr, adj = BR.build_graph(segment_len)
        ranks = BR.pagerank(rowptr, adj, 3)                                               # asserts the spread condition on every iteration
        assert ranks.dtype == np.float32 and (ranks > 0).all() and 0.5 < float(ranks.astype(np.float64).sum()) <= 1.0 + 1e-4
    ranks0 = BR.pagerank(rowptr, adj, 0)
    assert (ranks0 == np.float32(1.0 / BR.V)).all()
    # and it is a condition: terms spread over 30 binades fail it
    _, _, ok = BR.exact_f32_sum([1.0] * 1024 + [2.0 ** -30])
    assert not ok
    total, e, ok = BR.exact_f32_sum([0.5, 0.25, 2.0 ** -20])
    assert ok and Fraction(total) * Fraction(2) ** e == Fraction(3, 4) + Fraction(1, 1 << 20)


def test_value_families_meet_the_contract():
    """every family stays below the capacity and gives zero or normal sums (row_sums asserts it); the families are not vacuous"""
    rowptr, adj = BR.build_graph(65)
    seen = {}
    for name, bound, values in BR.value_families():
        be = BR.bound_exp_of(bound)
        acc, want = BR.row_sums(rowptr, adj, values, bound)
        assert max(acc) < 1 << 62, name
        finite = values[np.isfinite(values)]
        assert len(finite) == len(values) and (values[values != 0] > 0).all() and float(values.max()) < 2.0 ** be, name
        seen[name] = (acc, want, be)
    acc, want, _ = seen["ladder bound 1"]
    singles = [acc[BR.LADDER_ROW0 + j] for j in range(BR.LADDER_LEN)]
    assert singles[0] == 1 << 61 and singles[1] == 0xFFFFFF << 38
    assert singles[2 * 38] == 1 << 23 and singles[2 * 39] == 1 << 22                      # sh = 0, then -1
    assert singles[2 * 61] == 1 and singles[2 * 61 + 1] == 1 and singles[2 * 62] == 0 and singles[2 * 62 + 1] == 0       # sh = -23, then -24
    for k, expect in ((-40, 0.25), (-37, 0.25 + 2.0 ** -25)):
        acc, want, _ = seen["0.25 and 4096 of 2^%d" % k]
        assert float(want[BR.STAR_ROW]) == expect
    chain = np.float32(0.25)
    for _ in range(4096):
        chain = np.float32(chain + BR.pow2(-37))
    assert chain == np.float32(0.25), "an f32 chain loses every one of them"
    acc, want, be = seen["5000 truncated by 5, bound 1"]
    assert acc[BR.STAR_ROW] == 5000 * (0xFFFFFF >> 5)
    rounded = 5000 * ((0xFFFFFF + 16) >> 5)
    assert BR.round_once(rounded, be - 62) != want[BR.STAR_ROW], "the case tells a truncation from a rounding"
    assert seen["5000 truncated by 29, bound 1"][0][BR.STAR_ROW] == 0
    acc, want, _ = seen["subnormal inputs"]
    assert acc[BR.STAR_ROW] == 64 * (0x7FFFFF << 30) and float(want[BR.STAR_ROW]) >= 2.0 ** -126
    acc, want, _ = seen["signed zeros"]
    assert not any(acc) and (want.view(np.int32) == 0).all()
    acc, want, _ = seen["sum equal to 0.3, value below capacity"]
    assert want[BR.THREE_ROW0] == np.float32(0.3) and acc[BR.THREE_ROW0 + 3] == 0xFFFFFF << 38
