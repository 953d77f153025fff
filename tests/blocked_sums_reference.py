"""The blocked exact sums (csrc/pr.hip: vgl_pr_blk_op behind PR_BLOCKED, vgl_sum_blk_op behind vgl_hip_sum_over_edges_f32) restated in Python
integers: every f32 becomes an integer number of units of 2^(bound_exp - 62), integers add exactly, and the total is rounded to f32 ONCE.  No
device code and no floating-point accumulation: what the kernels promise ("the exact sum, rounded to f32 once, the same bits for any cut into
units") is what these functions compute, so the GPU tests compare int32 views for equality.

Also the test graph of tests/test_blocked_sums_gpu.py (build_graph), so that the CPU tests can check the conditions it has to meet."""
import math
from fractions import Fraction

import numpy as np

ACC_BLOCK = 16384          # ids per accumulate block of an operator with 8-byte accumulators
GATHER_BLOCK = 32768       # ids per gather block
CHUNK = 64                 # entries per chunk: a segment is padded to whole chunks


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def to_units(bits, bound_exp):
    """what one non-negative f32 (given by its bits) adds to an accumulator whose unit is 2^(bound_exp - 62): the mantissa with the hidden
    bit (exponent field 0 read as 1, without it) shifted by sh; a right shift truncates, and from 24 places on nothing is left"""
    bits = int(bits)
    ex = (bits >> 23) & 0xFF
    m = (bits & 0x7FFFFF) | (0x800000 if ex else 0)
    sh = (ex if ex else 1) - 150 + 62 - bound_exp
    if sh >= 0:
        return m << sh
    if sh <= -24:
        return 0
    return m >> -sh


def bound_exp_of(bound):
    """sums stay below 2^bound_exp: bound = m * 2^e with 0.5 <= m < 1 gives e + 1 (one spare bit), as in vgl_hip_sum_over_edges_f32"""
    return math.frexp(float(np.float32(bound)))[1] + 1


def round_once(acc, exp2):
    """acc * 2^exp2 (acc a non-negative integer) rounded to f32 once, to nearest, ties to even -- with integers only.  The result is 0 or a
    normal f32 (asserted: subnormal results are outside the tested contract)."""
    acc = int(acc)
    if acc == 0:
        return np.float32(0.0)
    drop = acc.bit_length() - 24
    if drop > 0:
        q, rem, half = acc >> drop, acc & ((1 << drop) - 1), 1 << (drop - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
        acc, exp2 = q, exp2 + drop                                        # q <= 2^24: exact in f32 at any exponent in range
    lo = exp2 + acc.bit_length() - 1                                      # exponent of the leading bit
    assert -126 <= lo <= 127, ("the expected sum is not a normal f32", acc, exp2)
    out = np.float32(math.ldexp(acc, exp2))
    assert Fraction(float(out)) == Fraction(acc) * Fraction(2) ** exp2
    return out


def double_rounded(acc, bound_exp):
    """the conversion before the fix: u64 -> f64 (a first rounding beyond 53 significant bits) -> f32.  Only to show where the two differ."""
    return np.float32(math.ldexp(float(int(acc)), bound_exp - 62))


def row_sums(rowptr, adj, values, bound):
    """per row the integer accumulator over the entries with adj != row (duplicates once each) and the expected f32 sums"""
    be = bound_exp_of(bound)
    units = [to_units(b, be) for b in np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).tolist()]
    rowptr, adj = np.asarray(rowptr).tolist(), np.asarray(adj).tolist()
    acc = [0] * (len(rowptr) - 1)
    for r in range(len(acc)):
        a = 0
        for e in range(rowptr[r], rowptr[r + 1]):
            if adj[e] != r:
                a += units[adj[e]]
        assert a < 1 << 64, ("row %d overflows a 64-bit accumulator" % r)
        acc[r] = a
    want = np.array([round_once(a, be - 62) for a in acc], dtype=np.float32)
    return acc, want


def indegree_noloops(rowptr, adj):
    rowptr, adj = np.asarray(rowptr), np.asarray(adj)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return np.bincount(adj[rows != adj], minlength=len(rowptr) - 1).astype(np.int64)


def exact_f32_sum(terms):
    """(integer, exponent) of the exact sum of f32 terms, and the spread condition under which a float64 sum of them is exact in ANY order:
    (largest - smallest exponent of the non-zero terms) + 24 + ceil(log2(count)) <= 53"""
    terms = [float(t) for t in terms if t != 0]
    if not terms:
        return 0, 0, True
    parts = [math.frexp(t) for t in terms]                                 # t = m * 2^e, 0.5 <= m < 1
    e_min, e_max = min(e for _, e in parts), max(e for _, e in parts)
    total = sum(int(math.ldexp(m, 24)) << (e - e_min) for m, e in parts)   # m * 2^24 is an integer for an f32 (subnormals included)
    assert all(math.ldexp(m, 24) == int(math.ldexp(m, 24)) for m, _ in parts)
    ok = (e_max - e_min) + 24 + math.ceil(math.log2(len(terms))) <= 53
    return total, e_min - 24, ok


def pagerank(rowptr, adj, iterations):
    """PR_BLOCKED step by step in f32 (vgl_k_pr_setup, vgl_k_pr_prepare, vgl_k_pr_dangling, vgl_pr_blk_op::finish), the per-row sums from
    row_sums at bound_exp = 0 (to_fixed: unit 2^-62) and the dangling term as the f32 of the exact sum of the f32 terms old / float(V).  The
    device forms that sum in float64 in an order of its own: the spread condition of exact_f32_sum, asserted on every iteration, is what makes
    it the exact sum whatever the order -- a condition on the inputs, not a tolerance."""
    V = len(rowptr) - 1
    indeg = indegree_noloops(rowptr, adj)
    rdeg = np.where(indeg == 0, 0.0, 1.0 / np.maximum(indeg, 1)).astype(np.float32)
    d = np.float32(0.85)
    k = np.float32((1.0 - np.float64(d)) / np.float64(np.float32(V)))
    ranks = np.full(V, np.float32(1.0 / V), dtype=np.float32)
    assert bound_exp_of(0.25) == 0
    for _ in range(iterations):
        contrib = (ranks * rdeg).astype(np.float32)
        terms = (ranks[indeg == 0] / np.float32(V)).astype(np.float32)
        total, e, ok = exact_f32_sum(terms)
        assert ok, "the dangling terms are spread too far for an order-independent float64 sum"
        dangling = round_once(total, e)
        _, sums = row_sums(rowptr, adj, contrib, 0.25)
        ranks = (k + d * (sums + dangling).astype(np.float32)).astype(np.float32)
    return ranks


# ---- the test graph ----
V = 3 * ACC_BLOCK + 1                      # gather blocks [0, 32768) [32768, 49153); accumulate blocks of 16384 ids and a last one of one id
CORNERS = (0, ACC_BLOCK - 1, ACC_BLOCK, GATHER_BLOCK - 1, V - 1)       # first / last rows of accumulate blocks 0, 1 and 3
CORNER_TARGETS = (0, GATHER_BLOCK - 1, GATHER_BLOCK, V - 1)
HUB, HUB_LEN = 100, 9000                   # block 0: cut into slabs under VGL_BLK_ACCUM_UNIT=64 (9000 entries = 141+ chunks)
TRIPLE_ROW = 5                             # lists the hub three times and the star row; the hub lists it back, so that none of the three heavy
                                           # rows is a dangling vertex (their ranks would spread the dangling terms too far, see pagerank)
STAR_ROW, STAR_LEAF0, STAR_LEN = ACC_BLOCK + 116, 21000, 5001          # one row over 5001 leaves of its own
LADDER_ROW0, LADDER_LEN = 1000, 180        # row LADDER_ROW0 + j lists the single vertex ladder_leaf(j)
THREE_ROW0, THREE_LEAF0, THREE_ROWS = 2100, 31000, 4                   # row THREE_ROW0 + j lists leaves THREE_LEAF0 + 3 j .. + 3 j + 2
SEGMENT_LENGTHS = (1, 63, 64, 65, 128)     # entries of row V - 1 into [32768, V): a segment of its own, at both sides of the 64-entry chunk


def ladder_leaf(j):
    return (20000 if j % 2 == 0 else 40000) + j                           # alternately in the first and the second gather block


def build_graph(segment_len):
    """(rowptr int64, adj int32).  Rows 32768 .. 49151 are empty, so accumulate block 2 has no edge; every corner row lists the four corner
    targets and itself (the self loops are dropped by the layout); row V - 1 lists segment_len ids of [32768, V) besides itself."""
    rows = {}
    for r in CORNERS:
        rows[r] = list(CORNER_TARGETS) + [r]
    rows[V - 1] += list(range(GATHER_BLOCK + 1, GATHER_BLOCK + segment_len))          # 32768 itself is a corner target: segment_len in all
    rows[TRIPLE_ROW] = [HUB, HUB, HUB, STAR_ROW]
    rows[HUB] = [TRIPLE_ROW] + list(range(3000, 7499)) + list(range(41000, 45500))    # both gather blocks, none of the leaves below
    assert len(rows[HUB]) == HUB_LEN
    rows[STAR_ROW] = list(range(STAR_LEAF0, STAR_LEAF0 + STAR_LEN))
    for j in range(LADDER_LEN):
        rows[LADDER_ROW0 + j] = [ladder_leaf(j)]
    for j in range(THREE_ROWS):
        rows[THREE_ROW0 + j] = [THREE_LEAF0 + 3 * j + i for i in range(3)]
    assert all(r < GATHER_BLOCK or r == V - 1 for r in rows)
    lengths = np.zeros(V, dtype=np.int64)
    for r, lst in rows.items():
        lengths[r] = len(lst)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    adj = np.concatenate([np.asarray(rows[r], dtype=np.int32) for r in sorted(rows)])
    assert len(adj) == rowptr[-1] <= 30000
    return rowptr, adj


# ---- the value families of the GPU test: (name, bound, values) with values an f32 array over the vertices of build_graph ----
def pow2(k):
    out = np.float32(math.ldexp(1.0, k))
    assert out != 0 and np.isfinite(out)
    return out


def base_values(seed=11):
    """values at every vertex, bound 1.0: integers below 2^20 times 2^-34 (exact in units of 2^-60; 9000 of them stay below 0.55), every 7th a
    full mantissa far down (0xFFFFFF * 2^-70: loses its low 10 bits), every 11th +0.0 and every 13th -0.0"""
    rng = np.random.default_rng(seed)
    v = (rng.integers(1, 1 << 20, V).astype(np.float32) * pow2(-34)).astype(np.float32)
    v[::7] = np.float32(0xFFFFFF) * pow2(-70)
    v[::11] = np.float32(0.0)
    v[::13] = np.float32(-0.0)
    return v


def ladder(bound):
    """one entry per row: 2^k and (2 - 2^-23) * 2^k for k = bound_exp - 1 down to bound_exp - 90, crossing sh = 0, -1, -23 and -24"""
    be, v = bound_exp_of(bound), np.zeros(V, dtype=np.float32)
    for j in range(LADDER_LEN // 2):
        k = be - 1 - j
        v[ladder_leaf(2 * j)] = pow2(k)
        v[ladder_leaf(2 * j + 1)] = np.float32(math.ldexp(2.0 - 2.0 ** -23, k))
        assert float(v[ladder_leaf(2 * j + 1)]) == math.ldexp(2.0 - 2.0 ** -23, k)
    return v


def star(first, rest, count):
    v = np.zeros(V, dtype=np.float32)
    v[STAR_LEAF0] = first
    v[STAR_LEAF0 + 1:STAR_LEAF0 + 1 + count] = rest
    assert count < STAR_LEN
    return v


def threes(*rows):
    v = np.zeros(V, dtype=np.float32)
    for j, row in enumerate(rows):
        for i, x in enumerate(row):
            assert float(np.float32(x)) == float(x), "not an f32"
            v[THREE_LEAF0 + 3 * j + i] = np.float32(x)
    return v


BOUNDS = (1.0, 0.3, 1000.0, 2.0 ** 60)
LARGEST_SUBNORMAL = np.array([0x007FFFFF], dtype=np.uint32).view(np.float32)[0]
# the double-rounding triple: 2^59 + 2^35 + 1 units of 2^-60 lies above the f32 tie, the double drops the 1 and the tie goes down to even;
# its mirror 2^59 + 2^36 + 2^35 - 1 lies below the tie, the double rounds up onto it and the tie goes up to even
TRIPLE = (0.5, 2.0 ** -25, 2.0 ** -60)
MIRROR = (0.5 + 2.0 ** -24, (2.0 ** 24 - 1) * 2.0 ** -49, (2.0 ** 11 - 1) * 2.0 ** -60)


def value_families():
    f32_03 = float(np.float32(0.3))
    fam = [("base", 1.0, base_values())]
    fam += [("ladder bound %g" % b, b, ladder(b)) for b in BOUNDS]
    fam += [("0.25 and 4096 of 2^%d" % k, 1.0, star(0.25, pow2(k), 4096)) for k in (-40, -37)]
    for b in (1.0, 1000.0):
        for down in (5, 24 + 5):                  # 5 bits lost per entry / as the issue states it: below one unit, every entry gone
            x = np.float32(0xFFFFFF) * pow2(bound_exp_of(b) - 62 - down)
            fam.append(("5000 truncated by %d, bound %g" % (down, b), b, star(x, x, 4999)))
    fam.append(("double rounding and mirror", 1.0, threes(TRIPLE, MIRROR)))
    fam.append(("subnormal inputs", 2.0 ** -119, star(LARGEST_SUBNORMAL, LARGEST_SUBNORMAL, 63)))
    zeros = np.zeros(V, dtype=np.float32)
    zeros[1::2] = np.float32(-0.0)
    fam.append(("signed zeros", 1.0, zeros))
    # a sum equal to a bound that is no power of two; a single value one ulp below 2^bound_exp = 1 (above the bound, below the capacity)
    fam.append(("sum equal to 0.3, value below capacity", 0.3, threes((f32_03 / 2, f32_03 / 2, -0.0), (), (), (float(np.nextafter(np.float32(1.0), np.float32(0.0))), 0.0, 0.0))))
    return fam
