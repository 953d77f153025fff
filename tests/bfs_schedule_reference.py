"""What the direction-optimising BFS must do, restated: a plain level-synchronous BFS on the stored multigraph (self loops and multi-edges kept)
whose direction per level follows the rule documented at vgl_do_turn_bottom_up / vgl_do_turn_top_down (vgl_hip_internal.h), in Python integers.
Nothing here knows of frontier states, hints or kernels: `schedule` yields the levels and one record per expanded level, `expected` the
statistics vgl_hip_bfs_run must report for them.

The second half builds the shaped inputs of tests/test_bfs_schedule_{cpu,gpu}.py: traversals that RMAT and uniform graphs never give (two
bottom-up phases, bottom-up from the first level, heavy levels that stay top-down, a graph with almost no rows that can be discovered, 3000 levels
of one vertex).  All are seeded, none has a vertex count that is a multiple of 64, all stay below 40 000 vertices and 1.2 M entries."""
from collections import namedtuple

import numpy as np

ALPHA, BETA = 15, 18
TOP_DOWN, BOTTOM_UP = "t", "B"

# F / M: size and out-degree sum of the level's frontier; found: vertices it discovers; unvisited_in_entries: in-entries of the rows that are
# unvisited when the level starts (what a bottom-up level could probe at most once each)
Level = namedtuple("Level", "level direction F M found unvisited_in_entries")


def do_factor(V, E):
    return max(1, E // V // 2)


def turn_bottom_up(F, M, prev_f, visited, V, factor):
    """`visited` counts the frontier about to be expanded"""
    return F > prev_f and M >= ((V - visited) * factor + V) // ALPHA


def turn_top_down(F, prev_f, visited, V, factor):
    return F <= prev_f and F < ((V - visited) * factor + V) // (factor * BETA)


def schedule(V, src, dst, source, direction_optimising=True):
    """(levels, [Level, ...]): source at level 1, unreached rows -1"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    E = len(src)
    out_deg, in_deg = np.bincount(src, minlength=V), np.bincount(dst, minlength=V)
    start = np.concatenate([[0], np.cumsum(out_deg)])
    adj = dst[np.argsort(src, kind="stable")]
    factor = do_factor(V, E)
    levels = np.full(V, -1, np.int32)
    levels[source] = 1
    frontier = np.array([source], np.int64)
    level, prev_f, visited, bottom_up, records = 1, 0, 0, False, []
    unvisited_in = int(in_deg.sum()) - int(in_deg[source])
    while len(frontier):
        F, M = len(frontier), int(out_deg[frontier].sum())
        visited += F
        if direction_optimising:
            if not bottom_up:
                bottom_up = turn_bottom_up(F, M, prev_f, visited, V, factor)
            elif turn_top_down(F, prev_f, visited, V, factor):
                bottom_up = False
        # every entry of the frontier's rows, whichever direction reads it
        first = np.repeat(start[frontier] - np.concatenate([[0], np.cumsum(out_deg[frontier])[:-1]]), out_deg[frontier])
        heads = adj[first + np.arange(M)]
        found = np.unique(heads[levels[heads] < 0])
        levels[found] = level + 1
        records.append(Level(level, BOTTOM_UP if bottom_up else TOP_DOWN, F, M, len(found), unvisited_in))
        unvisited_in -= int(in_deg[found].sum())
        prev_f, frontier, level = F, found, level + 1
    return levels, records


def expected(records):
    """the statistics of vgl_hip_bfs_stats that the schedule fixes (a last level that finds nothing is a step like any other)"""
    td = [r for r in records if r.direction == TOP_DOWN]
    bu = [r for r in records if r.direction == BOTTOM_UP]
    total = sum(r.F for r in records)
    return dict(levels=len(records), discovered=total, frontier_total=total, td_steps=len(td), bu_steps=len(bu),
                td_frontier=sum(r.F for r in td), td_edges=sum(r.M for r in td), bu_found=sum(r.found for r in bu))


STATS = tuple(expected([]))


def directions(records):
    """run-length form, e.g. "t3 B2 t53 B2 t1" """
    runs = []
    for r in records:
        if runs and runs[-1][0] == r.direction:
            runs[-1][1] += 1
        else:
            runs.append([r.direction, 1])
    return " ".join("%s%d" % (d, n) for d, n in runs)


def phases(records):
    """the bottom-up phases: lists of consecutive bottom-up records"""
    out, inside = [], False
    for r in records:
        if r.direction == BOTTOM_UP:
            if not inside:
                out.append([])
            out[-1].append(r)
        inside = r.direction == BOTTOM_UP
    return out


def switches_back(records):
    """the first top-down record after each bottom-up phase"""
    return [b for a, b in zip(records, records[1:]) if a.direction == BOTTOM_UP and b.direction == TOP_DOWN]


def in_nz_rows(V, dst):
    return int((np.bincount(np.asarray(dst, np.int64), minlength=V) > 0).sum())


# ---- shaped inputs: each returns (V, src, dst, source), int32 arrays ----
def _cluster(rng, first, n, degree):
    return np.repeat(np.arange(first, first + n), degree), rng.integers(first, first + n, n * degree)


def _pack(V, parts, source):
    src = np.concatenate([np.asarray(s, np.int64) for s, _ in parts]).astype(np.int32)
    dst = np.concatenate([np.asarray(d, np.int64) for _, d in parts]).astype(np.int32)
    assert V % 64 != 0 and V < 40000 and len(src) < 1200000 and 0 <= src.min() and max(src.max(), dst.max()) < V and 0 <= dst.min()
    return V, src, dst, source


def two_bursts(seed=1, n=8000, degree=16, path=50):
    """two random clusters joined by a directed path that leaves the first cluster's source: each cluster is one bottom-up phase, the path
    between them 50 levels of one vertex"""
    rng = np.random.default_rng(seed)
    p0, b0 = n, n + path
    chain = np.arange(p0, p0 + path)
    return _pack(2 * n + path, [_cluster(rng, 0, n, degree), ([0], [p0]), (chain[:-1], chain[1:]), ([chain[-1]], [b0]),
                                _cluster(rng, b0, n, degree)], 0)


def hub_source(seed=2, V=20011):
    """the source has an entry to every other vertex: the first level is bottom-up"""
    rng = np.random.default_rng(seed)
    return _pack(V, [(np.zeros(V - 1, np.int64), np.arange(1, V)), (np.repeat(np.arange(V), 2), rng.integers(0, V, 2 * V))], 0)


def hub_layer(seed=3, hubs=40, fan=1500, body=30000):
    """source -> 40 hubs -> a body of out-degree 2: level 2 is a small frontier with many entries"""
    rng = np.random.default_rng(seed)
    h0, b0 = 1, 1 + hubs
    return _pack(1 + hubs + body, [(np.zeros(hubs, np.int64), np.arange(h0, b0)),
                                   (np.repeat(np.arange(h0, b0), fan), rng.integers(b0, b0 + body, hubs * fan)),
                                   (np.repeat(np.arange(b0, b0 + body), 2), rng.integers(b0, b0 + body, 2 * body))], 0)


def heavy_not_growing(width=400, layers=8, closed=False):
    """0 -> 1 -> a layer of `width` by single entries, a matching into a second layer of `width`, then complete bipartite layers of width - 1,
    width - 2, ...: `layers` layers after the first.  No frontier grows once the entries become many, so no level turns bottom-up.
    closed: the last layer has an entry to every vertex of the layer before it (a heavy level that discovers nothing)."""
    sizes = [width, width] + [width - k for k in range(1, layers)]
    firsts = 2 + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    ids = [np.arange(f, f + s) for f, s in zip(firsts, sizes)]
    parts = [([0], [1]), (np.ones(width, np.int64), ids[0]), (ids[0], ids[1])]
    for a, b in zip(ids[1:] + ([ids[-1]] if closed else []), ids[2:] + ([ids[-2]] if closed else [])):
        parts.append((np.repeat(a, len(b)), np.tile(b, len(a))))
    return _pack(2 + sum(sizes), parts, 0)


def heavy_not_growing_shrunk():
    return heavy_not_growing(width=120)


def late_from_start(seed=5, V=32771, core=400):
    """only `core` rows have incoming entries: 8 from every other vertex, 60 each among themselves"""
    rng = np.random.default_rng(seed)
    outer = np.arange(core, V)
    return _pack(V, [(np.repeat(outer, 8), rng.integers(0, core, 8 * len(outer))),
                     (np.repeat(np.arange(core), 60), rng.integers(0, core, 60 * core))], V - 1)


def deep_path(n=3000, isolated=500):
    return _pack(n + isolated, [(np.arange(n - 1), np.arange(1, n))], 0)


# ---- the rule's inequalities at their boundaries, as graphs (factor 1: fewer than 4 V entries) ----
def _pack_small(V, parts, source):
    out = _pack(V, parts, source)
    assert do_factor(V, len(out[1])) == 1
    return out


def bottom_up_boundary(short, V=2003, hubs=10):
    """0 -> 10 hubs -> a body: level 2 has F = 10 > 1 and M = the bottom-up threshold - `short`.  Every body vertex has one entry to a vertex
    of its own, so that the direction of the levels shows in the statistics."""
    M = ((V - (1 + hubs)) + V) // ALPHA - short
    body = 1 + hubs + np.arange(M)
    return _pack_small(V, [(np.zeros(hubs, np.int64), 1 + np.arange(hubs)), (1 + np.arange(M) % hubs, body), (body, body + M)], 0)


def top_down_boundary(short, V=2003, first=300):
    """0 -> 300 vertices (bottom-up from level 1, and level 2 grows), of which the first f have one entry each to a vertex of their own: level 3 has
    F = f <= prevF, with f the smallest frontier that does NOT turn top-down (`short` = 0) or one less, the largest that does (`short` = 1)"""
    def threshold(f):
        return ((V - (1 + first + f)) + V) // BETA
    f = next(f for f in range(1, first) if f >= threshold(f)) - short
    mid = 1 + first + np.arange(f)
    return _pack_small(V, [(np.zeros(first, np.int64), 1 + np.arange(first)), (1 + np.arange(f), mid), (mid, mid + f)], 0)


def equal_frontiers(V=2003, width=100):
    """0 -> 100 vertices by three entries each (bottom-up from level 1), then two more levels of 100 by single entries: level 3 has F == prevF,
    which is `not growing` and turns top-down"""
    a = 1 + np.arange(width)
    return _pack_small(V, [(np.zeros(3 * width, np.int64), np.tile(a, 3)), (a, a + width), (a + width, a + 2 * width)], 0)


def burst(seed=7, n=4000, degree=16):
    return _pack(n, [_cluster(np.random.default_rng(seed), 0, n, degree)], 0)


# the four ways a traversal ends, and a component whose traversal ends that way inside `endings_union`
ENDINGS = (("list_kernel_finishes", lambda: deep_path(300, 0)),             # every level fits the list kernel, the last one included
           ("bitmap_expand_finds_nothing", burst),                          # bottom-up, then a small top-down level that discovers nothing
           ("empty_count_after_top_down", lambda: heavy_not_growing(120, closed=True)),    # the last level is heavy and discovers nothing
           ("bottom_up_finds_nothing", hub_source),                         # bottom-up from the first level to the last
           ("source_without_entries", None))                                # one vertex: a level without entries and nothing after it


def endings_union():
    """the components of ENDINGS side by side in one graph: (V, src, dst, {ending: source})"""
    base, parts, sources = 0, [], {}
    for name, make in ENDINGS:
        V, src, dst, source = make() if make else (1, np.zeros(0, np.int32), np.zeros(0, np.int32), 0)
        parts.append((src.astype(np.int64) + base, dst.astype(np.int64) + base))
        sources[name] = base + source
        base += V
    return _pack(base, parts, sources)


SHAPES = dict(two_bursts=two_bursts, hub_source=hub_source, hub_layer=hub_layer, heavy_not_growing=heavy_not_growing,
              late_from_start=late_from_start, deep_path=deep_path, heavy_not_growing_shrunk=heavy_not_growing_shrunk,
              bottom_up_at_threshold=lambda: bottom_up_boundary(0), bottom_up_below_threshold=lambda: bottom_up_boundary(1),
              top_down_at_threshold=lambda: top_down_boundary(0), top_down_below_threshold=lambda: top_down_boundary(1),
              equal_frontiers=equal_frontiers)


def study_graph(seed, log_v_end=22):
    """the generator of tests/studies/fuzz_bfs.py (skewed / uniform, sparse / dense, isolated vertices, self loops, multi-edges, every fifth
    seed a path glued on) with fewer than 2^(log_v_end - 1) vertices; returns (V, src, dst, rng) with the stream where the study leaves it"""
    rng = np.random.default_rng(991000 + seed)
    V = int(rng.integers(2, 1 << int(rng.integers(8, log_v_end))))
    E = int(rng.integers(0, int(rng.choice([1, 2, 8, 32])) * V + 1))
    e1, e2 = float(rng.choice([1, 1, 2, 4, 8])), float(rng.choice([1, 1, 2, 4, 8]))
    src = np.minimum((rng.random(E) ** e1 * V).astype(np.int32), V - 1)
    dst = np.minimum((rng.random(E) ** e2 * V).astype(np.int32), V - 1)
    if seed % 5 == 0 and E:
        n = min(V - 1, 3000)
        src = np.concatenate([src, np.arange(n, dtype=np.int32)])
        dst = np.concatenate([dst, np.arange(1, n + 1, dtype=np.int32)])
    return V, src, dst, rng
