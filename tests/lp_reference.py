"""Sequential restatement of the label propagation contract of include/vgl_hip.h (vgl_hip_lp_run), vectorised with numpy.

Test support, not a test file: tests/test_lp_cpu.py checks it on hand-made cases, tests/test_lp_gpu.py compares the HIP path with it.
"""
import numpy as np

LP_DEFAULT_MAX_ITERATIONS = 20        # lp.h:10


def lp_step(rowptr, adj, labels):
    """one synchronous iteration: the most frequent label among each row's entries, ties to the largest label; empty rows keep theirs"""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int32)
    V = rowptr.size - 1
    deg = np.diff(rowptr)
    rows = np.repeat(np.arange(V, dtype=np.int64), deg)
    nb = labels[np.asarray(adj, dtype=np.int64)] if rows.size else np.zeros(0, dtype=np.int32)
    out = labels.copy()
    if rows.size == 0:
        return out
    order = np.lexsort((nb, rows))                        # by row, then label
    r, lab = rows[order], nb[order]
    start = np.ones(r.size, dtype=bool)
    start[1:] = (r[1:] != r[:-1]) | (lab[1:] != lab[:-1])
    first = np.flatnonzero(start)
    run_row, run_lab = r[first], lab[first]
    run_cnt = np.diff(np.append(first, r.size))
    pick = np.lexsort((run_lab, run_cnt, run_row))        # per row ascending (count, label): the row's last run wins
    pr = run_row[pick]
    last = np.ones(pr.size, dtype=bool)
    last[:-1] = pr[1:] != pr[:-1]
    out[pr[last]] = run_lab[pick][last]
    return out


def label_propagation(rowptr, adj, init=None, max_iterations=LP_DEFAULT_MAX_ITERATIONS):
    """returns (labels, iterations, changed_history): stops after the first iteration that changes nothing (counted) or at the cap"""
    V = len(rowptr) - 1
    labels = np.arange(V, dtype=np.int32) if init is None else np.array(init, dtype=np.int32)
    history = []
    for _ in range(max_iterations):
        nxt = lp_step(rowptr, adj, labels)
        changed = int(np.count_nonzero(nxt != labels))
        history.append(changed)
        labels = nxt
        if changed == 0:
            break
    return labels, len(history), history


def csr_from_edges(V, src, dst):
    """stable CSR (rows by source, entries in input order) of an edge list"""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int32)
    order = np.argsort(src, kind="stable")
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.add.at(rowptr, src + 1, 1)
    return np.cumsum(rowptr), dst[order]


I32_MIN, I32_MAX = -2**31, 2**31 - 1


def _both(edges):
    return edges + [(b, a) for a, b in edges]


# hand-checked cases: name -> (V, edges (src, dst), init labels or None, max_iterations, expected labels, iterations, changed history)
HAND_CASES = {
    "path": (5, _both([(0, 1), (1, 2), (2, 3), (3, 4)]), None, 2, [2, 3, 4, 3, 4], 2, [5, 5]),
    "star": (5, _both([(0, 1), (0, 2), (0, 3), (0, 4)]), None, 20, [0, 4, 4, 4, 4], 20, [5] * 20),
    "bridged_triangles": (6, _both([(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3)]), None, 20, [3, 3, 3, 5, 5, 5], 4, [6, 4, 1, 0]),
    "k22_oscillates": (4, _both([(0, 2), (0, 3), (1, 2), (1, 3)]), None, 5, [3, 3, 1, 1], 5, [4] * 5),
    "self_loop": (2, [(0, 0), (0, 1), (1, 1), (1, 0)], [5, 7], 20, [7, 7], 2, [1, 0]),
    "multi_edge": (4, [(0, 1), (0, 2), (0, 2), (0, 3)], None, 20, [2, 1, 2, 3], 2, [1, 0]),
    "isolated_vertex": (3, [(0, 1), (1, 0)], [10, 20, -5], 3, [20, 10, -5], 3, [2, 2, 2]),
    "all_equal_start": (6, _both([(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3)]), [7] * 6, 20, [7] * 6, 1, [0]),
    "extreme_ties": (6, [(0, 1), (0, 2), (3, 4), (3, 5)], [0, I32_MIN, I32_MAX, 0, -2, -1], 20, [I32_MAX, I32_MIN, I32_MAX, -1, -2, -1], 2, [2, 0]),
    "int32_min_majority": (5, _both([(0, 1), (0, 2), (0, 3), (0, 4)]), [0, I32_MIN, I32_MIN, I32_MAX, -1], 1, [I32_MIN, 0, 0, 0, 0], 1, [5]),
}
