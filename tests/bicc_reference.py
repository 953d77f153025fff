"""Sequential restatement of the biconnectivity contract of include/vgl_hip.h (vgl_hip_bicc_run) in plain Python / numpy, on
tri_reference.simple_undirected and ktruss_reference.edge_list: an iterative depth-first search with lowpoints and an edge stack (Hopcroft and Tarjan).
It shares nothing with the library's method (a BFS forest, subtree intervals and union-finds), so the two sides are independent.

Test support, not a test file: tests/test_bicc_cpu.py checks it on hand-made cases and against networkx, tests/test_bicc_gpu.py compares the HIP path
with it.
"""
import numpy as np

from ktruss_reference import edge_list

INT_STATS = ("undirected_edges", "components", "bridges", "articulation_points", "biconnected_components", "two_edge_components",
             "largest_component_edges", "depth")


def biconnected(V, src, dst):
    """dict: edge_u, edge_v int32[E'] (ascending (lo, hi)), bridge bool[E'], edge_component int32[E'] (the smallest edge id of the block),
    articulation bool[V], two_edge_component int32[V] (the smallest vertex id of the component of graph minus bridges), and the INT_STATS"""
    A, eu, ev = edge_list(V, src, dst)
    A = A.tocsr()
    A.sort_indices()
    E = int(eu.size)
    indptr, indices = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(indptr))
    keys = eu.astype(np.int64) * V + ev
    slot_eid = np.searchsorted(keys, np.minimum(rows, indices) * V + np.maximum(rows, indices)).tolist()
    ptr, adj = indptr.tolist(), indices.tolist()

    disc, low = [-1] * V, [0] * V
    block = [-1] * E
    bridge = np.zeros(E, dtype=bool)
    art = np.zeros(V, dtype=bool)
    clock = nblocks = components = 0
    for root in range(V):
        if disc[root] >= 0:
            continue
        components += 1
        disc[root] = low[root] = clock
        clock += 1
        root_children = 0
        stack = [(root, -1, ptr[root])]          # (vertex, the edge it was entered by, the next slot of its row)
        estack = []
        while stack:
            v, pe, at = stack[-1]
            if at < ptr[v + 1]:
                stack[-1] = (v, pe, at + 1)
                w, e = adj[at], slot_eid[at]
                if e == pe:
                    continue
                if disc[w] < 0:
                    disc[w] = low[w] = clock
                    clock += 1
                    estack.append(e)
                    stack.append((w, e, ptr[w]))
                    if v == root:
                        root_children += 1
                elif disc[w] < disc[v]:          # a back edge, seen from its lower end
                    estack.append(e)
                    if disc[w] < low[v]:
                        low[v] = disc[w]
                continue
            stack.pop()
            if not stack:
                break
            u = stack[-1][0]
            if low[v] < low[u]:
                low[u] = low[v]
            if low[v] >= disc[u]:                # u separates the subtree of v: the edges above (u, v) on the stack are one block
                if u != root:
                    art[u] = True
                members = []
                while True:
                    e = estack.pop()
                    members.append(e)
                    if e == pe:
                        break
                name = min(members)
                for e in members:
                    block[e] = name
                nblocks += 1
            if low[v] > disc[u]:
                bridge[pe] = True
        if root_children >= 2:
            art[root] = True

    # the 2-edge-connected components: a union-find over the edges that are no bridges, the smallest id as the name
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for e in np.flatnonzero(~bridge).tolist():
        a, b = find(int(eu[e])), find(int(ev[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
    two = np.array([find(v) for v in range(V)], dtype=np.int32)

    # depth: a BFS from the smallest vertex of every component
    level = [-1] * V
    depth = 0
    for root in range(V):
        if level[root] >= 0:
            continue
        level[root] = 0
        front = [root]
        while front:
            depth = max(depth, level[front[0]] + 1)
            nxt = []
            for v in front:
                for w in adj[ptr[v]:ptr[v + 1]]:
                    if level[w] < 0:
                        level[w] = level[v] + 1
                        nxt.append(w)
            front = nxt
    block = np.asarray(block, dtype=np.int32).reshape(E)
    sizes = np.bincount(block, minlength=1) if E else np.zeros(1, dtype=np.int64)
    return {"edge_u": eu, "edge_v": ev, "bridge": bridge, "edge_component": block, "articulation": art, "two_edge_component": two,
            "undirected_edges": E, "components": components, "bridges": int(bridge.sum()), "articulation_points": int(art.sum()),
            "biconnected_components": nblocks, "two_edge_components": int(np.unique(two).size), "largest_component_edges": int(sizes.max()),
            "depth": depth}


def algorithmic_bytes(V, E, depth, edges=True, bridge=True, blocks=True, two_edge=True):
    """the bytes model of include/vgl_hip.h, for the outputs asked for"""
    nnz = 2 * E
    return (92 * V + 16 * nnz + 24 * E + 104 * (depth + 1) + (16 * E if edges else 0) + (E if bridge else 0) + (33 * V + 20 * E + 8 * nnz if blocks else 0) +
            (12 * V if two_edge else 0))


def _clique(n, first=0):
    return [(first + a, first + b) for a in range(n) for b in range(a + 1, n)]


def _tree(depth):
    """complete binary tree with `depth` levels below the root: vertex i has the children 2 i + 1 and 2 i + 2"""
    n = (1 << (depth + 1)) - 1
    return n, [((i - 1) // 2, i) for i in range(1, n)]


def _case(V, stored, bridges, cuts, blocks, two_edge):
    """(V, stored entries, expected: bridges as (lo, hi), cut vertices, blocks as sets of (lo, hi), the 2-edge-connected components as sets)"""
    return V, stored, {"bridges": sorted(bridges), "cuts": sorted(cuts), "blocks": sorted(sorted(b) for b in blocks), "two_edge": sorted(sorted(c) for c in two_edge)}


def _singletons(V, but=()):
    seen = {v for c in but for v in c}
    return [list(c) for c in but] + [[v] for v in range(V) if v not in seen]


_P6 = [(i, i + 1) for i in range(5)]
_C6 = [(i, (i + 1) % 6) for i in range(6)]
_BOWTIE = _clique(4) + _clique(4, 3)                                   # two K4 that share vertex 3
_BARBELL = _clique(4) + _clique(4, 4) + [(3, 4)]
_THETA = [(0, 2), (2, 1), (0, 3), (3, 4), (4, 1), (0, 5), (5, 6), (6, 7), (7, 1)]      # three paths from 0 to 1
_LADDER = [(i, i + 1) for i in range(4)] + [(5 + i, 6 + i) for i in range(4)] + [(i, 5 + i) for i in range(5)]
_TREE4 = _tree(4)
# the case the non-local rule exists for: 0 - 1 is a bridge into p = 1, whose children 2 and 3 carry the subtrees {2, 4} and {3, 5}, joined by the
# cross edge 4 - 5 and by nothing else.  p is a cut vertex; the tree edges of 2 and 3 are one block (the cycle 1 2 4 5 3), whichever parents a forest picks
_CROSS = [(0, 1), (1, 2), (1, 3), (2, 4), (3, 5), (4, 5)]


def _sorted_edges(edges):
    return sorted((min(a, b), max(a, b)) for a, b in edges)


# name -> (V, stored entries (src, dst), expected values written out)
HAND_CASES = {
    # a handle holds at least one vertex: the empty graph is the graph without an edge on the fewest vertices
    "empty": _case(1, [], [], [], [], [[0]]),
    "isolated_vertices": _case(5, [], [], [], [], _singletons(5)),
    "only_loops": _case(4, [(0, 0), (2, 2), (2, 2)], [], [], [], _singletons(4)),
    "one_edge_stored_three_times": _case(2, [(0, 1), (1, 0), (0, 1)], [(0, 1)], [], [[(0, 1)]], [[0], [1]]),
    "path_6": _case(6, _P6, _P6, [1, 2, 3, 4], [[e] for e in _P6], _singletons(6)),
    "cycle_6": _case(6, _C6, [], [], [_sorted_edges(_C6)], [list(range(6))]),
    "k5": _case(5, _clique(5), [], [], [_clique(5)], [list(range(5))]),
    "bowtie": _case(7, _BOWTIE, [], [3], [_clique(4), _clique(4, 3)], [list(range(7))]),
    "barbell": _case(8, _BARBELL, [(3, 4)], [3, 4], [_clique(4), _clique(4, 4), [(3, 4)]], [[0, 1, 2, 3], [4, 5, 6, 7]]),
    "theta": _case(8, _THETA, [], [], [_sorted_edges(_THETA)], [list(range(8))]),
    "ladder_2x5": _case(10, _LADDER, [], [], [_sorted_edges(_LADDER)], [list(range(10))]),
    "binary_tree_4": _case(_TREE4[0], _TREE4[1], _TREE4[1], list(range(15)), [[e] for e in _TREE4[1]], _singletons(_TREE4[0])),
    "cross_edge_below_a_cut_vertex": _case(6, _CROSS, [(0, 1)], [1], [[(0, 1)], _sorted_edges(_CROSS[1:])], [[0], [1, 2, 3, 4, 5]]),
}


def expected_arrays(V, stored, want):
    """the hand case's expectation as the arrays of biconnected(): (bridge, edge_component, articulation, two_edge_component)"""
    simple = sorted({(min(a, b), max(a, b)) for a, b in stored if a != b})
    at = {e: i for i, e in enumerate(simple)}
    bridge = np.zeros(len(simple), dtype=bool)
    bridge[[at[e] for e in want["bridges"]]] = True
    block = np.full(len(simple), -1, dtype=np.int32)
    for b in want["blocks"]:
        ids = [at[tuple(e)] for e in b]
        block[ids] = min(ids)
    art = np.zeros(V, dtype=bool)
    art[want["cuts"]] = True
    two = np.full(V, -1, dtype=np.int32)
    for c in want["two_edge"]:
        two[c] = min(c)
    return bridge, block, art, two


def block_graph(seed, blocks, hub_share):
    """(V, src, dst, expected counts): `blocks` blocks glued at cut vertices, so that the counts are known BY CONSTRUCTION.  Start with vertex 0; every
    block attaches at vertex 0 with probability hub_share, otherwise at a uniformly chosen existing vertex, and is a single edge, a cycle of 3 - 12, a
    clique of 3 - 8 or a ring of 8 - 40 with as many random chords; new vertices make up the rest of the block.  Every edge is stored in a random
    orientation, an antiparallel copy is added with probability 0.1, a parallel one with 0.05, a loop with 0.02; five isolated vertices are appended
    and all ids go through a random permutation."""
    rng = np.random.default_rng(seed)
    n = 1
    edges = []
    in_blocks = {0: 0}
    single = 0
    for _ in range(blocks):
        at = 0 if rng.random() < hub_share else int(rng.integers(0, n))
        kind = int(rng.integers(0, 4))
        k = 2 if kind == 0 else int(rng.integers(3, 13)) if kind == 1 else int(rng.integers(3, 9)) if kind == 2 else int(rng.integers(8, 41))
        vs = [at] + list(range(n, n + k - 1))
        n += k - 1
        for v in vs:
            in_blocks[v] = in_blocks.get(v, 0) + 1
        if kind == 0:
            edges.append((vs[0], vs[1]))
            single += 1
        elif kind == 2:
            edges += [(vs[a], vs[b]) for a in range(k) for b in range(a + 1, k)]
        else:
            edges += [(vs[i], vs[(i + 1) % k]) for i in range(k)]
            if kind == 3:
                for _ in range(k):
                    a, b = int(rng.integers(0, k)), int(rng.integers(0, k))
                    if a != b:
                        edges.append((vs[a], vs[b]))
    stored = []
    for a, b in edges:
        if rng.random() < 0.5:
            a, b = b, a
        stored.append((a, b))
        if rng.random() < 0.1:
            stored.append((b, a))
        if rng.random() < 0.05:
            stored.append((a, b))
        if rng.random() < 0.02:
            stored.append((a, a))
    V = n + 5
    perm = rng.permutation(V)
    s = perm[np.asarray([a for a, _ in stored], dtype=np.int64)]
    d = perm[np.asarray([b for _, b in stored], dtype=np.int64)]
    expect = {"biconnected_components": blocks, "bridges": single, "articulation_points": sum(1 for c in in_blocks.values() if c >= 2),
              "two_edge_components": single + 1 + 5, "components": 6}
    return V, s.astype(np.int64), d.astype(np.int64), expect
