"""Adversarial edge weights / capacities for the shortest-path and widest-path schedules, and plain numpy restatements of the two fixed points.

Test support, not a test file: tests/test_sssp_weights_cpu.py proves on the CPU that the oracle's Bellman-Ford, its second algorithm (Dijkstra / the
worklist) and the restatements below agree in every bit on these inputs; tests/test_sssp_weights_gpu.py then compares every HIP schedule with the oracle.

The contract under test is finite, non-negative float32 weights whose path sums stay finite.  On that domain fl(d + w) is monotone in d and never
below d, so the least fixed point of d[v] = min(d[v], fl(d[u] + w)) does not depend on the evaluation order; widest paths only take min / max of
their inputs.  Bit equality is therefore the assertion everywhere.

Weights are produced in the order of the input COO; the tests carry them to CSR order with the build's permutation, as every other test does.
"""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
F32 = np.float32


def _uniform_0_100(rng, E):
    """k * 100 / 2^24 for a uniform 24-bit k >= 1: the suite's usual distribution without its (rare) zero"""
    return (rng.integers(1, 1 << 24, E).astype(np.float32) * F32(100.0 / 16777216.0)).astype(np.float32)


def _zeros(rng, E):
    return np.zeros(E, np.float32)


def _ones(rng, E):
    return np.ones(E, np.float32)


def _sparse_zeros(rng, E):
    w = _uniform_0_100(rng, E)
    w[rng.permutation(E)[: E // 2]] = 0.0
    return w


def _small_ints(rng, E):
    return rng.integers(0, 4, E).astype(np.float32)


def _two_values(rng, E):
    below = np.nextafter(F32(16.0), F32(0.0))
    return np.where(rng.integers(0, 2, E) == 1, F32(16.0), below).astype(np.float32)


def _denormals(rng, E):
    return rng.integers(0, 1 << 20, E).astype(np.int32).view(np.float32).copy()       # the bit pattern k IS k * 2^-149 below 2^23


def _tiny(rng, E):
    return ((rng.integers(1, 1 << 24, E).astype(np.float32) * F32(1.0 / 16777216.0)) * F32(1e-30)).astype(np.float32)


def _wide_range(rng, E):
    return np.ldexp(F32(1.0), rng.integers(-140, 61, E).astype(np.int32)).astype(np.float32)


def _top_of_domain(rng, E):
    w = _uniform_0_100(rng, E)
    w[rng.permutation(E)[: E // 2]] = np.nextafter(F32(100.0), F32(0.0))
    return w


def _flt_max_some(rng, E):
    w = _uniform_0_100(rng, E)
    w[rng.permutation(E)[: max(1, E // 10)]] = FLT_MAX
    return w


WEIGHT_CLASSES = {
    "zeros": _zeros,
    "ones": _ones,
    "sparse_zeros": _sparse_zeros,
    "small_ints": _small_ints,
    "two_values": _two_values,
    "denormals": _denormals,
    "tiny": _tiny,
    "wide_range": _wide_range,
    "top_of_domain": _top_of_domain,
}

CAPACITY_CLASSES = {
    "zeros": _zeros,
    "ones": _ones,
    "sparse_zeros": _sparse_zeros,
    "flt_max_some": _flt_max_some,
    "denormals": _denormals,
    "wide_range": _wide_range,
}


def make(classes, name, E, seed):
    """float32[E] of class `name`, in input-COO order; the stream depends on (class, seed) only"""
    rng = np.random.default_rng([int(seed), sorted(classes).index(name), len(classes)])
    w = classes[name](rng, int(E))
    assert w.dtype == np.float32 and w.shape == (E,) and np.isfinite(w).all() and (w >= 0).all()
    return w


def sssp_numpy(V, src, dst, w, source):
    """edge-list Bellman-Ford, every operation in float32: Jacobi sweeps of d[dst] = min(d[dst], d[src] + w) until nothing changes.  Unreached
    vertices keep FLT_MAX (FLT_MAX + w == FLT_MAX for every w of the domain)."""
    dist = np.full(V, FLT_MAX, np.float32)
    dist[source] = 0.0
    w = np.asarray(w, np.float32)
    while True:
        new = dist.copy()
        np.minimum.at(new, dst, dist[src] + w)
        assert new.dtype == np.float32
        if np.array_equal(new.view(np.int32), dist.view(np.int32)):
            return dist
        dist = new


def sswp_numpy(V, src, dst, cap, source):
    """the same for widest paths: width[dst] = max(width[dst], min(width[src], cap)); source FLT_MAX, unreached 0"""
    width = np.zeros(V, np.float32)
    width[source] = FLT_MAX
    cap = np.asarray(cap, np.float32)
    while True:
        new = width.copy()
        np.maximum.at(new, dst, np.minimum(width[src], cap))
        if np.array_equal(new.view(np.int32), width.view(np.int32)):
            return width
        width = new


def csr_sources(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int32), np.diff(rowptr))


def ring_with_chords(V):
    """directed ring 0 -> 1 -> ... -> V-1 -> 0 with a chord v -> (7 v + 3) mod V from every fifth vertex: strongly connected, deep and narrow
    frontiers (many buckets in sequence)"""
    v = np.arange(V, dtype=np.int64)
    c = v[::5]
    src = np.concatenate([v, c])
    dst = np.concatenate([(v + 1) % V, (7 * c + 3) % V])
    return src.astype(np.int32), dst.astype(np.int32)


def _generated(O, kind, scale, ef, seed):
    src, dst = (O.gen_rmat if kind == "rmat" else O.gen_uniform)(scale, ef, seed)
    return {"name": "%s_s%d_e%d" % (kind, scale, ef), "V": 1 << scale, "src": src, "dst": dst, "seed": seed}


def _ring(V, seed):
    src, dst = ring_with_chords(V)
    return {"name": "ring_%d" % V, "V": V, "src": src, "dst": dst, "seed": seed}


def graphs(O):
    """the graphs of the class x schedule tests: the smallest that still reach each kernel family (O: the oracle module, for its generators)"""
    return [_generated(O, "rmat", 12, 16, 3), _generated(O, "ru", 13, 8, 5), _ring(300, 7)]


def small_graphs(O):
    """for the extreme deltas: a denormal delta makes a bucket of (nearly) every distinct distance"""
    return [_ring(1 << 10, 11), _generated(O, "rmat", 10, 8, 2)]


def block_pair_graph(O):
    """two 16384-id blocks: the least at which the blocked layouts have a block pair"""
    return _generated(O, "rmat", 15, 16, 13)


def delta_plan_edges(rowptr, adj, w, delta, place_le=False, first_writer_wins=False):
    """(src, dst, w) of the edges that a delta plan holds: light part then heavy part, both stable.  The flags and their scan use w < delta.
    place_le models the seeded mistake of the sensitivity check -- the partition alone places by w <= delta: an edge with w == delta then
    lands on the light slot of the next light edge (which of the two writers stays is a race: first_writer_wins) and leaves its heavy slot
    unwritten (modelled as an edge to vertex 0 of weight 0).  With place_le=False this is a permutation of the input edges."""
    E, V, delta = len(adj), len(rowptr) - 1, np.float32(delta)
    S = np.concatenate([[0], np.cumsum(w < delta)]).astype(np.int64)
    n_light = int(S[E])
    a = [np.zeros(n_light + 1, np.int32), np.zeros(E - n_light + 1, np.int32)]
    v = [np.zeros(n_light + 1, np.float32), np.zeros(E - n_light + 1, np.float32)]
    e = np.arange(E)
    to_light = (w <= delta) if place_le else (w < delta)
    order = e[to_light][::-1] if first_writer_wins else e[to_light]
    a[0][S[order]], v[0][S[order]] = adj[order], w[order]
    heavy = e[~to_light]
    a[1][heavy - S[heavy]], v[1][heavy - S[heavy]] = adj[heavy], w[heavy]
    rows = np.arange(V, dtype=np.int32)
    src = np.concatenate([np.repeat(rows, np.diff(S[rowptr])), np.repeat(rows, np.diff(rowptr - S[rowptr]))])
    return src, np.concatenate([a[0][:n_light], a[1][:E - n_light]]), np.concatenate([v[0][:n_light], v[1][:E - n_light]])
