"""Inputs of the pull-sum tests (vectorgraphlibrary_amd/csrc/vgl_pull.h: PageRank's ordered f32 chain, HITS' chunked f64 sums) and the shape
arithmetic that says which of the kernel's four paths a row reaches.

Test support, not a test file: tests/test_pull_rows_cpu.py proves with numpy that the rows sit on the batch, round, chunk and tile boundaries they
are meant for and that a wrong summation order or a lost entry changes the bits; tests/test_pull_rows_gpu.py feeds them to the kernels.  Every
graph is (V, src, dst) with int32 ids, deterministic, no random draws.  Within a row the adjacency order equals the input order (stable CSR build).

The constants restate vgl_pull.h and vgl_hip_internal.h.
"""
import numpy as np

HUB_DEGREE = 512          # rows at least this long leave the one-thread-per-row path
HUB_BATCH = 512           # values a hub wavefront folds per batch
NP = 3                    # producer wavefronts of a giant workgroup = batches per round
CHUNK = 4096              # entries per chunk of the unordered (HITS) hub sums
GIANT_DEGREE = 32768
GIANT_BLOCKS = 64
HUB_BLOCKS = 256
TILE = 2048
BLOCK = 256
BLOCK_EDGES = 16384
WAVES = 4

# ---- vertex layout of the ladder (every region starts on a multiple of 256, so region = row group) ----
LADDER_V = 390 * BLOCK + 3                 # a final partial group of exactly 3 rows
G_511 = 0                                  # 256 rows of 511 entries: 8 parts
G_16384 = 256                              # 256 rows of 64 entries: exactly BLOCK_EDGES, 1 part
G_16385 = 512                              # one entry more: 2 parts
G_STRADDLE = 768                           # rows placed by in-block offset
G_UNROLL = 1024                            # lengths 1 .. 17, one copy per self-loop position
G_PLACE = 1280                             # hubs first / last / mid-tile / adjacent in a block of short rows
G_LONG = 1536                              # the named long rows on even ids, 3-entry rows between them
G_IN = 1792                                # targets of the in-direction ladder (two groups)
PEERS = (4096, 32768)                      # (first vertex, count): neighbours of the rows under test, entries 0 .. 512 of a row
LIGHT = (36864, 8192)                      # entries 513 and later of a long row (crafted_values)
SOURCES = (45056, 16384)                   # sources of the in-direction ladder
FILLER = (61440, LADDER_V - 3 - 61440)     # every FILLER_EVERY-th vertex has a row of 1 .. 5 entries, the others none
FILLER_EVERY = 16

LONG_LENGTHS = (511, 512, 513, 514, 515, 1023, 1024, 1025, 1536, 1537, 2047, 2049, 3072, 3073, 3585, 4097)


def loop_positions(n):
    return sorted({p for p in (0, 511, 512, n - 1) if p < n})


EXTRA_LENGTHS = tuple(range(513, 583))     # with VGL_PULL_GIANT_DEGREE=513: 70 + ... > 64 giants
GIANT_LENGTHS = (32767, 32768, 32769, 33281)   # 64, 64, 65, 66 batches, 22 rounds each; the 40000-entry tail hub has 79 batches, 27 rounds (odd)
TAIL_HUB = 40000
UNROLL_MAX = 17
IN_LENGTHS = (512, 513, 700, 4095, 4096, 4097, 8192, 8193, 12289)
IN_EXTRA = 250                             # further 512-entry in-rows: more than 256 hubs in the in-direction
SHARD_BOUNDS = (0, G_PLACE, PEERS[0] + 192, LADDER_V)   # the middle shard starts with the hub of G_PLACE and owns the long rows with self loops


def block_rows(rowptr):
    """(blk_row, parts per 256-row group) as vgl_pull_find_hubs cuts them: a group is halved until a part holds about BLOCK_EDGES entries, while
    every part keeps at least two rows; step = ceil(rows / parts)"""
    nrows = len(rowptr) - 1
    blk, parts_of = [], []
    for r0 in range(0, nrows, BLOCK):
        r1 = min(nrows, r0 + BLOCK)
        e = int(rowptr[r1] - rowptr[r0])
        parts = 1
        while parts < 32 and e > BLOCK_EDGES * parts and (r1 - r0) >= 2 * parts:
            parts *= 2
        step = -(-(r1 - r0) // parts)
        blk.extend(range(r0, r1, step))
        parts_of.append(parts)
    blk.append(nrows)
    return np.asarray(blk, dtype=np.int64), np.asarray(parts_of, dtype=np.int64)


def hub_counts(rowptr, giant_degree=GIANT_DEGREE):
    """(hubs, giants, chunks of the unordered variant) of one direction"""
    deg = np.diff(rowptr)
    hubs = deg[deg >= HUB_DEGREE]
    return int(hubs.size), int((hubs >= giant_degree).sum()), int((-(-hubs // CHUNK)).sum())


def batches_and_rounds(n):
    nb = -(-n // HUB_BATCH)
    return nb, -(-nb // NP)


# ---- crafted in-degrees and the f32 chain of iteration 1 ----
def crafted_values(v):
    """magnitudes 1 .. 2^20 cycling with the vertex id (neighbouring ids: 4 binades apart, scrambled mantissas), one id in 16 zero.  Every other
    stretch of 1024 ids has its values doubled, so the sum over a window of 511 consecutive ids halves and doubles again as the window moves and
    crosses a power of two on the way: _Builder.row needs such starts.  The LIGHT peers (entries 513 and later of a long row) cycle through
    2^12 .. 2^20 only: what a long row adds after its first batch stays below the binade the first batch reached -- a chain that keeps doubling
    rounds away, at its end, whatever the order of entries 511 and 512 did to it."""
    v = np.asarray(v, dtype=np.int64)
    light = (v >= LIGHT[0]) & (v < LIGHT[0] + LIGHT[1])
    k = np.where(light, 12 + (v * 4) % 9, (v * 4) % 21)
    val = ((np.int64(1) << k) * (1024 + (v * 40503) % 1024)) >> 10
    val = np.minimum(np.where(((v // 1024) % 2 == 1) & ~light, 2 * val + 1, val), 1 << 20)
    return np.where(v % 16 == 11, 0, val).astype(np.int32)


def crafted_indeg(V, under_test):
    """int32[V]: crafted_values everywhere but on the rows under test themselves, which get 1, 2 or 3 (a self loop summed by mistake then weighs
    about as much as the largest entries of the chain)"""
    out = crafted_values(np.arange(V))
    under_test = np.asarray(under_test, dtype=np.int64)
    out[under_test] = 1 + under_test % 3
    return out


def first_contrib(V, indeg):
    """contrib of iteration 1 (pr.hip: vgl_k_pr_setup + vgl_k_pr_prepare): f32(1/V) * f32(1/indeg), or 0"""
    rdeg = np.where(indeg == 0, 0.0, 1.0 / np.maximum(indeg, 1)).astype(np.float32)
    return np.float32(1.0 / V) * rdeg


def chain_f32(terms):
    """the sequential f32 `+=` chain from 0 (np.cumsum adds one element at a time in the array's type)"""
    terms = np.asarray(terms, dtype=np.float32)
    return np.float32(0) if terms.size == 0 else np.cumsum(terms, dtype=np.float32)[-1]


def wrong_variants(v, entries):
    """name -> the ENTRIES a wrong kernel would sum for row v, in its order (the caller still drops the self loops, except for `self_included`);
    a variant that does not exist for the row is left out"""
    n = entries.size
    out = {"reversed": entries[::-1], "last_dropped": entries[:n - 1]}
    if n > HUB_BATCH:
        out["tail_dropped"] = entries[:(n // HUB_BATCH) * HUB_BATCH]
        sw = entries.copy()
        sw[[511, 512]] = sw[[512, 511]]
        out["swapped_511_512"] = sw
    if (entries == v).any():
        out["self_included"] = entries
    return out


def summed(v, entries, contrib, keep_self=False):
    return contrib[entries] if keep_self else contrib[entries[entries != v]]


def discriminates(v, entries, contrib):
    """name -> True / False / None: the f32 chain of the variant differs in bits from the right chain; None where the variant sums the very same
    sequence (the dropped or swapped entries are self loops, or fewer than three terms are reversed) and so cannot differ"""
    right_terms = summed(v, entries, contrib)
    right = chain_f32(right_terms).view(np.int32)
    res = {}
    for name, e in wrong_variants(v, entries).items():
        terms = summed(v, e, contrib, keep_self=(name == "self_included"))
        if name == "reversed" and right_terms.size < 3:
            res[name] = None                      # a + b == b + a in any rounding: nothing to tell apart
        elif terms.size == right_terms.size and (terms.view(np.int32) == right_terms.view(np.int32)).all():
            res[name] = None
        else:
            res[name] = bool(chain_f32(terms).view(np.int32) != right)
    return res


# ---- the ladder ----
class _Builder:
    def __init__(self, V):
        self.V = V
        self.rows = {}                            # vertex -> int64 array of neighbours, in adjacency order
        self.in_edges = []                        # (sources, target)
        self.names = {}
        self.cursor = 0                           # next first peer to try
        self.contrib = first_contrib(V, crafted_values(np.arange(V)))   # of the peers (the rows under test are never peers)
        self.heavy = np.tile(self.contrib[PEERS[0]:PEERS[0] + PEERS[1]].astype(np.float64), 2)      # wrapped once: windows of 513 from any start
        self.prefix = np.concatenate([[0.0], np.cumsum(self.heavy)])

    def name(self, case, v):
        self.names.setdefault(case, []).append(int(v))

    def peers(self, first, n):
        i = np.arange(n, dtype=np.int64)
        return np.where(i <= HUB_BATCH, PEERS[0] + (first + i) % PEERS[1], LIGHT[0] + (first + i) % LIGHT[1])

    def put(self, v, entries):
        assert v not in self.rows
        self.rows[int(v)] = np.asarray(entries, dtype=np.int64)

    def row(self, v, n, loops=(), tuned=True):
        """n distinct consecutive peers with self loops at the positions `loops`; tuned: the first peer is the first one from the cursor on for
        which every wrong variant that can differ does differ (the chain of iteration 1 under the crafted in-degrees).
        Swapping two neighbouring terms changes an f32 chain only where the running sum changes its binade between them (within one binade every
        term is rounded to the same grid whatever the order), so a row longer than a batch is placed where the sum crosses a power of two at
        entries 511 / 512: the starts where it may (f64 prefix sums, with a margin for the chain's own error) are listed first, one in a few hundred."""
        loops = np.asarray(loops, dtype=np.int64)
        starts = (self.cursor + np.arange(PEERS[1] if tuned else 1)) % PEERS[1]
        if tuned and n > HUB_BATCH and 511 not in loops and 512 not in loops:
            c = self.heavy
            before = self.prefix[starts + 511] - self.prefix[starts] - sum(c[starts + p] for p in loops if p < 511)
            after = before + c[starts + 511] + c[starts + 512]
            starts = starts[np.frexp(before * (1 - 1e-4))[1] != np.frexp(after * (1 + 1e-4))[1]]
        self.contrib[v] = np.float32(1.0 / self.V) * np.float32(1.0 / (1 + v % 3))
        for first in starts:
            e = self.peers(int(first), n)
            e[loops] = v
            if not tuned or all(d is not False for d in discriminates(v, e, self.contrib).values()):
                break
        else:
            raise AssertionError("no first peer found for row %d (%d entries)" % (v, n))
        self.cursor = (int(first) + 61) % PEERS[1]
        self.put(v, e)


def ladder():
    """(V, src, dst, rows): rows maps a case name to the vertex ids under test (see the module docstring of tests/test_pull_rows_cpu.py)"""
    V = LADDER_V
    b = _Builder(V)
    # ordinary rows
    for i in range(BLOCK):
        b.row(G_511 + i, 511, tuned=False)
        b.name("group_511", G_511 + i)
        b.row(G_16384 + i, 64, tuned=False)
        b.name("group_16384", G_16384 + i)
        b.row(G_16385 + i, 65 if i == 100 else 64, tuned=False)
        b.name("group_16385", G_16385 + i)
    # in-block offsets: 4 x 511 = 2044, +3 = 2047, the straddling row [2047, 2049), 4 x 511 = 4093, +3 = 4096, an empty row at 4096, 5 more
    v = G_STRADDLE
    for n, case in [(511, None)] * 4 + [(3, None), (2, "straddle")] + [(511, None)] * 4 + [(3, None), (0, "empty_at_tile"), (5, "after_empty")]:
        if n:
            b.row(v, n, tuned=False)
        if case:
            b.name(case, v)
        b.name("group_straddle", v)
        v += 1
    v = G_UNROLL
    for n in range(1, UNROLL_MAX + 1):
        for p in range(n):
            b.row(v, n, loops=(p,))
            b.name("unroll", v)
            v += 1
    b.row(v, 10, loops=(4, 5))
    b.name("adjacent_loops", v)
    # hub placement: 7-entry rows around a hub that opens its block, one that starts mid-tile, two in a row (the second spans a tile), one that closes it
    placed = {G_PLACE: ("hub_first", 600, (0, 599)), G_PLACE + 120: ("hub_mid_tile", 700, ()), G_PLACE + 170: ("hubs_adjacent", 600, (5,)),
              G_PLACE + 171: ("hubs_adjacent", 1500, ()), G_PLACE + BLOCK - 1: ("hub_last", 513, (512,))}
    for i in range(BLOCK):
        v = G_PLACE + i
        if v in placed:
            case, n, loops = placed[v]
            b.row(v, n, loops=loops)
            b.name(case, v)
        else:
            b.row(v, 7, loops=(3,) if i % 5 == 0 else (), tuned=False)
            b.name("group_place_short", v)
    # the named long rows
    long_rows = []
    for n in LONG_LENGTHS:
        long_rows += [("len%d" % n, n, ()), ("len%d_loops" % n, n, tuple(loop_positions(n)))]
    long_rows += [("all_loops_600", 600, tuple(range(600))), ("one_loop_512", 512, (100,))]
    long_rows += [("extra_513_582", n, ()) for n in EXTRA_LENGTHS]
    long_rows += [("giant_%d" % n, n, (0, 511, 512, n - 1) if n == 32769 else ()) for n in GIANT_LENGTHS]
    assert len(long_rows) <= BLOCK // 2
    for i in range(BLOCK):
        v = G_LONG + i
        if i % 2 == 0 and i // 2 < len(long_rows):
            case, n, loops = long_rows[i // 2]
            b.row(v, n, loops=loops)
            b.name(case, v)
        else:
            b.row(v, 3, loops=(1,) if i % 7 == 0 else (), tuned=False)
    # the final partial group: 3 rows, the middle one a hub longer than two parts' worth of entries
    b.row(V - 3, 9, loops=(8,))
    b.row(V - 2, TAIL_HUB, loops=(0, 511, 512, TAIL_HUB - 1))
    b.row(V - 1, 4)
    for v in (V - 3, V - 2, V - 1):
        b.name("tail_group", v)
    b.name("tail_hub", V - 2)
    # peers and filler: short rows of their own, so ranks differ from the second iteration on.  Their targets are spread unevenly (a modulus that
    # changes from row to row): tens of thousands of vertices with one and the same value make the sequential sum of squares of oracle.hits drift
    # by 1e-12 (every addition rounds the same way), which would use up the HITS tolerance before any kernel is looked at
    skew = lambda i, n, count: (i * 31 + 17 * np.arange(n, dtype=np.int64) + 5) % (1 + (i * 7919) % count)
    for i in range(PEERS[1]):
        if i % 4:
            b.put(PEERS[0] + i, PEERS[0] + skew(i, i % 4, PEERS[1]))
    for i in range(0, FILLER[1], FILLER_EVERY):   # (the other filler rows are empty: a zero adds exactly)
        b.put(FILLER[0] + i, FILLER[0] + skew(i, 1 + (i // FILLER_EVERY) % 5, FILLER[1]))
    # in-direction: every target is pointed at by n distinct sources, one entry each (the sources scattered by a permutation of their range:
    # neighbouring sources then have different targets and different sums)
    for j, n in enumerate(IN_LENGTHS + (512,) * IN_EXTRA):
        t = G_IN + j
        b.in_edges.append((SOURCES[0] + ((j * 1237 + np.arange(n, dtype=np.int64)) * 7919) % SOURCES[1], t))
        b.name("in_len%d" % n if j < len(IN_LENGTHS) else "in_extra_512", t)
    src_parts, dst_parts, pos_parts = [], [], []
    extra = {}
    for s, t in b.in_edges:
        for u in s:
            extra.setdefault(int(u), []).append(t)
    for u, ts in extra.items():
        b.put(u, np.asarray(ts, dtype=np.int64))
    for v in sorted(b.rows):
        e = b.rows[v]
        src_parts.append(np.full(e.size, v, dtype=np.int64))
        dst_parts.append(e)
        pos_parts.append(np.arange(e.size, dtype=np.int64))
    src, dst, pos = np.concatenate(src_parts), np.concatenate(dst_parts), np.concatenate(pos_parts)
    # input order: all first entries, then all second entries, ... -- far from CSR order, the order WITHIN a row kept (the stable build restores it)
    order = np.argsort(pos, kind="stable")
    rows = {k: np.asarray(vs, dtype=np.int64) for k, vs in b.names.items()}
    return V, src[order].astype(np.int32), dst[order].astype(np.int32), rows


def chain_rows(rows):
    """the vertex ids whose ordered chain the tests pin: the named long rows, the placed hubs, the tail hub"""
    keys = [k for k in rows if k.startswith(("len", "giant_", "extra_", "hub", "tail_hub", "one_loop", "all_loops"))]
    return np.concatenate([rows[k] for k in sorted(keys)])


def under_test(rows):
    return np.unique(np.concatenate([chain_rows(rows), rows["unroll"], rows["adjacent_loops"], rows["tail_group"]]))


def case_of(rows, v):
    return sorted(k for k, ids in rows.items() if v in ids) or ["(unnamed)"]


# ---- small graphs ----
def single_vertex_hub():
    return 1, np.zeros(600, np.int32), np.zeros(600, np.int32)


def two_vertices():
    return 2, np.zeros(513, np.int32), np.ones(513, np.int32)


def one_hub():
    """one hub (row 7, 700 entries, self loops at both ends and at 511 / 512) among 3-entry rows: one hub workgroup, three of its wavefronts idle"""
    V = 300
    hub = 8 + np.arange(700, dtype=np.int64) % 200
    hub[[0, 511, 512, 699]] = 7
    others = np.array([v for v in range(V) if v != 7], dtype=np.int64)
    src = np.concatenate([np.full(700, 7, dtype=np.int64), np.repeat(others, 3)])
    dst = np.concatenate([hub, (np.repeat(others, 3) * 5 + np.tile(np.arange(3), others.size) * 11) % V])
    return V, src.astype(np.int32), dst.astype(np.int32)


SMALL = {"single_vertex_hub": single_vertex_hub, "two_vertices": two_vertices, "one_hub": one_hub}


# ---- the unordered (HITS) order of additions ----
def seq_row_sums(rowptr, adj, x, rows):
    """f64 `+=` chains in adjacency order for the given rows (all shorter than HUB_DEGREE), one vectorised add per position"""
    rows = np.asarray(rows, dtype=np.int64)
    deg = rowptr[rows + 1] - rowptr[rows]
    order = np.argsort(-deg, kind="stable")
    rows, deg = rows[order], deg[order]
    acc = np.zeros(rows.size, dtype=np.float64)
    for j in range(int(deg.max()) if rows.size else 0):
        m = int(np.searchsorted(-deg, -j, side="left"))       # rows with deg > j come first
        acc[:m] = acc[:m] + x[adj[rowptr[rows[:m]] + j]]
    return rows, acc


def chunk_sum(vals):
    """vgl_pull_hub_chunks on one chunk of at most CHUNK f64 values: lane l adds entries l + 256 t + 64 u into part[u] over the trips t,
    (p0 + p1) + (p2 + p3), then the butterfly over xor 32 .. 1; lane 0's value"""
    buf = np.zeros(CHUNK, dtype=np.float64)
    buf[:vals.size] = vals
    trips = buf.reshape(CHUNK // 256, 4, 64)
    part = np.zeros((4, 64), dtype=np.float64)
    for t in range(trips.shape[0]):
        part = part + trips[t]
    acc = (part[0] + part[1]) + (part[2] + part[3])
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    return acc[0]


def pull_unordered(rowptr, adj, x):
    """out[v] = sum of x over row v in the order of vgl_k_pull_sum<double, ORDERED = false>: chains below HUB_DEGREE, chunk sums added in order above"""
    V = len(rowptr) - 1
    deg = np.diff(rowptr)
    out = np.zeros(V, dtype=np.float64)
    rows, acc = seq_row_sums(rowptr, adj, x, np.flatnonzero(deg < HUB_DEGREE))
    out[rows] = acc
    for r in np.flatnonzero(deg >= HUB_DEGREE):
        a = np.float64(0)
        for c0 in range(int(rowptr[r]), int(rowptr[r + 1]), CHUNK):
            a = a + chunk_sum(x[adj[c0:min(c0 + CHUNK, int(rowptr[r + 1]))]])
        out[r] = a
    return out


def hits_unordered(out_csr, in_csr, steps):
    import math
    V = len(out_csr[0]) - 1
    auth, hub = np.ones(V), np.ones(V)
    for _ in range(steps):
        auth = pull_unordered(in_csr[0], in_csr[1], hub)
        auth = auth / math.sqrt(math.fsum(auth * auth))
        hub = pull_unordered(out_csr[0], out_csr[1], auth)
        hub = hub / math.sqrt(math.fsum(hub * hub))
    return auth, hub
