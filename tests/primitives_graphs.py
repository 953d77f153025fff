"""Inputs of the operator-primitive self-check (apps/primitives_contract.cpp) and the shape arithmetic that says which kernel branch an input reaches.

Test support, not a test file: tests/test_primitives_graphs_cpu.py proves with numpy that the graphs have the properties the branches need,
tests/test_primitives_contract_gpu.py feeds them to the program.  Every graph is (V, src, dst) with int32 ids, deterministic, no random draws.

The constants restate vectorgraphlibrary_amd/csrc/vgl_hip_internal.h and hip/vgl_hip_kernels.hpp: edge tiles of 2048, workgroups of 256 rows,
at most 1024 staged frontier positions per sparse tile, 4096-entry chunks of the sequential-rows advance, 1024 workgroups of a reduce.
"""
import math

import numpy as np

TILE = 2048
BLOCK = 256
STAGE = 1024
CHUNK = 4096
REDUCE_GRID = 1024
WAVE = 64
COMBINED_MIN_LANES = 8

RAGGED_V = REDUCE_GRID * BLOCK + 77
EMPTY_ENDS = 100                                   # vertices [0, 100) and [V - 100, V) have no edges in either direction
HUBS = ((1000, 5000, 9000), (1001, 9000, 5000))    # (vertex, entries of its outgoing row, entries of its incoming row)
HUB_PEERS = 10000                                  # hub k's peers: HUB_PEERS + 2 * i + k
MIXED = (2000, 6000)                               # (first vertex, count): rows of 1 .. 7 entries next to rows of 8 .. 63
MIXED_DEGREES = (3, 20, 1, 45, 7, 8, 63, 2, 30, 5, 12, 4)
MIXED_ROTATE = 5                                   # in-degree of the i-th vertex = MIXED_DEGREES[(i + 5) % 12]: no vertex has the same degree both ways
STRETCH = (100000, 60000)                          # (first vertex, count): degrees cycle 0, 1, 1, 0, 1, 2 in both directions
STRETCH_DEGREES = (0, 1, 1, 0, 1, 2)
STRETCH_ROTATE = 2                                 # the incoming cycle starts two steps later: 1, 0, 1, 2, 0, 1
LOOPS = (50000, 8)                                 # self loops, each stored twice
DUPLICATES = ((50020, 50021, 3), (50021, 50020, 2), (50022, 50022, 1))


def _matched(first, count, pattern, stride, rotate):
    """edges among `count` consecutive vertices (a multiple of len(pattern)) with out-degree pattern[i % len] and in-degree pattern[(i + rotate) % len]:
    the k-th entry of the source list (ids repeated by out-degree) meets entry (k * stride) % n of the target list (ids repeated by in-degree), a
    permutation because gcd(stride, n) == 1"""
    assert count % len(pattern) == 0
    ids = first + np.arange(count, dtype=np.int64)
    pattern = np.asarray(pattern, dtype=np.int64)
    sources = np.repeat(ids, pattern[np.arange(count) % pattern.size])
    targets = np.repeat(ids, pattern[(np.arange(count) + rotate) % pattern.size])
    n = sources.size
    while math.gcd(stride, n) != 1:
        stride += 1
    return sources, targets[(np.arange(n, dtype=np.int64) * stride + 17) % n]


def ragged():
    V = RAGGED_V
    parts = [_matched(MIXED[0], MIXED[1], MIXED_DEGREES, 7919, MIXED_ROTATE), _matched(STRETCH[0], STRETCH[1], STRETCH_DEGREES, 104729, STRETCH_ROTATE)]
    for k, (hub, out_entries, in_entries) in enumerate(HUBS):
        peers = lambda n: HUB_PEERS + 2 * np.arange(n, dtype=np.int64) + k
        parts += [(np.full(out_entries, hub, dtype=np.int64), peers(out_entries)), (peers(in_entries)[::-1], np.full(in_entries, hub, dtype=np.int64))]
    loops = LOOPS[0] + np.arange(LOOPS[1], dtype=np.int64)
    parts += [(loops, loops), (loops, loops)]
    for s, d, times in DUPLICATES:
        parts.append((np.full(times, s, dtype=np.int64), np.full(times, d, dtype=np.int64)))
    src = np.concatenate([p[0] for p in parts])
    dst = np.concatenate([p[1] for p in parts])
    # interleave the parts so that the input order is not the CSR order (the stable CSR build has something to do)
    order = np.argsort((np.arange(src.size, dtype=np.int64) * 48271) % 65537, kind="stable")
    return V, src[order].astype(np.int32), dst[order].astype(np.int32)


def tiny():
    return 1, np.zeros(1, np.int32), np.zeros(1, np.int32)


def no_edges():
    return 5, np.zeros(0, np.int32), np.zeros(0, np.int32)


def three_edges():
    return 70, np.array([3, 69, 3], np.int32), np.array([69, 0, 3], np.int32)


GRAPHS = {"ragged": ragged, "tiny": tiny, "no_edges": no_edges, "three_edges": three_edges}


# ---- the shape arithmetic ----
def csr(V, src, dst):
    """rows by source, entries in input order (the stable build of VGL_Graph::import)"""
    src = np.asarray(src, dtype=np.int64)
    order = np.argsort(src, kind="stable")
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=V), out=rowptr[1:])
    return rowptr, np.asarray(dst, dtype=np.int64)[order]


def both_directions(V, src, dst, fmt="csr"):
    """(outgoing CSR, incoming CSR) as VGL_Graph::import stores them: the incoming one is built from the outgoing CSR's list transposed.  fmt "vcsr":
    vertices renumbered by total degree first (largest first, ties by id)"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    if fmt == "vcsr":
        total = np.bincount(src, minlength=V) + np.bincount(dst, minlength=V)
        fwd = np.empty(V, dtype=np.int64)
        fwd[np.argsort(-total, kind="stable")] = np.arange(V)
        src, dst = fwd[src], fwd[dst]
    out = csr(V, src, dst)
    rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(out[0]))
    return out, csr(V, out[1], rows)


def frontier_ids(V, kind):
    v = np.arange(V, dtype=np.int64)
    return v[v % 7 == 0] if kind == "sparse" else v[v % 11 != 0] if kind == "large" else v


def sparse_tile_spans(rowptr, ids):
    """frontier positions per 2048-edge tile of a sparse advance, as the plan computes them: exclusive prefix sums of the active rows' degrees; the
    plan's table holds per tile the position that owns edge t * 2048 and, one past the tiles, the owner of the last edge; the kernel maps the
    positions from its tile's entry to the next entry (vgl_k_advance_sparse: np = p_last - p_first + 1)"""
    deg = rowptr[ids + 1] - rowptr[ids]
    offs = np.concatenate([[0], np.cumsum(deg)])
    M = int(offs[-1])
    if M == 0:
        return np.zeros(0, dtype=np.int64)
    owner = lambda e: np.searchsorted(offs, e, side="right") - 1
    table = np.concatenate([owner(np.arange(0, M, TILE, dtype=np.int64)), [owner(M - 1)]])
    return table[1:] - table[:-1] + 1


def unstaged_tiles(rowptr, ids):
    return int((sparse_tile_spans(rowptr, ids) > STAGE).sum())


def long_rows(rowptr):
    return int((np.diff(rowptr) > CHUNK).sum())


def multi_chunk_blocks(rowptr):
    V = rowptr.size - 1
    b = np.arange(0, V, BLOCK)
    return int((rowptr[np.minimum(b + BLOCK, V)] - rowptr[b] > CHUNK).sum())


def wave_kinds(rowptr):
    """(wavefronts of an all-active tile advance whose lanes all add to one source and are at least 8, wavefronts with more than one source): a
    wavefront handles 64 consecutive CSR positions starting at a multiple of 64"""
    E = int(rowptr[-1])
    if E == 0:
        return 0, 0
    rows = np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))
    first = np.arange(0, E, WAVE)
    last = np.minimum(first + WAVE, E) - 1
    same = rows[first] == rows[last]
    return int((same & (last - first + 1 >= COMBINED_MIN_LANES)).sum()), int((~same).sum())


def coverage(rowptr, V):
    """the coverage facts the program prints for one direction, from the CSR alone"""
    combined, mixed = wave_kinds(rowptr)
    return {
        "unstaged_sparse_tiles": unstaged_tiles(rowptr, frontier_ids(V, "sparse")),
        "rows_longer_than_chunk": long_rows(rowptr),
        "row_blocks_over_one_chunk": multi_chunk_blocks(rowptr),
        "combined_add_wavefronts": combined,
        "mixed_add_wavefronts": mixed,
    }
