"""Shaped inputs for tests/test_bfs_reach_rows_{cpu,gpu}.py: graphs whose vertices with incoming entries are numbered first, so that
reach_rows (1 + the largest vertex with an incoming entry) falls where the test wants it, and what the fused BFS does on them restated on the
CPU: does a traversal reach the scan of `levels` (vgl_k_bfs_scan_bound) and turn bottom-up right after it?

Every shape is a `core` [0, R) -- a ring plus 20 random entries per row, so every core vertex has incoming entries and R is reach_rows -- and,
numbered after it, vertices that have 30 entries into the core and no incoming one (`near`: before the end of the 2048-row tile that R falls
into; `far`, `far2`: after it, in a tile the bounded scan does not launch) and vertices without any entry (`isolated`, the last one).  From
such an entry the levels hold 1, 30, ~600, ... vertices: level 2 has too many entries for the list kernel and too few to turn bottom-up,
level 3 turns bottom-up."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfs_schedule_reference as R  # noqa: E402

TILE = 2048
Shape = namedtuple("Shape", "V src dst reach_rows sources")      # sources: {kind: vertex}

# name: (R, V): R in the middle of a byte (and of the second tile), of a 64-bit word, of a tile on a word boundary; inside the first tile (two
# tiles not launched); R == V with V no multiple of 64
LAYOUT = dict(mid_byte=(2051, 4500), mid_word=(2272, 4500), mid_tile=(3072, 4500), first_tile=(1000, 4500), whole=(4133, 4133))
SCAN_ENV = ({"VGL_TD_EMIT_EDGES": "0"}, {"VGL_TD_EMIT_EDGES": "0", "VGL_BFS_SMALL_M": "0"})


def shape(name, seed=11):
    core, V = LAYOUT[name]
    rng = np.random.default_rng(seed)
    rows = np.arange(core)
    parts = [(rows, (rows + 1) % core), (np.repeat(rows, 20), rng.integers(0, core, 20 * core))]
    tile_end = -(-core // TILE) * TILE
    sources = {"inside": 5}
    if V > core:
        entries = {"near": core + 1, "far": tile_end + 37, "far2": tile_end + 38}
        for kind, v in entries.items():
            assert core <= v < V - 1
            parts.append((np.full(30, v), rng.integers(0, core, 30)))
        sources.update(entries, isolated=V - 1)
    src = np.concatenate([s for s, _ in parts]).astype(np.int32)
    dst = np.concatenate([d for _, d in parts]).astype(np.int32)
    return Shape(V, src, dst, int(dst.max()) + 1, sources)


SCAN_BLOCKS = 1024         # VGL_SCAN_BLOCKS (bfs.hip): with more tiles than this a workgroup of the scan takes several, two per trip


def many_tiles(seed=12):
    """more vertex tiles below reach_rows than the scan has workgroups, and a ragged last one: a core of 1100.5 tiles with three random entries
    per row (no ring: a few core rows have no incoming entry, reach_rows is read off the arrays), the same entries and isolated vertex after it"""
    core = 1100 * TILE + 1027
    V = core + 4100
    rng = np.random.default_rng(seed)
    tile_end = -(-core // TILE) * TILE
    sources = {"inside": int(core // 2), "near": core + 1, "far": tile_end + 37, "far2": tile_end + 38, "isolated": V - 1}
    parts = [(np.repeat(np.arange(core), 3), rng.integers(0, core, 3 * core))]
    for kind in ("near", "far", "far2"):
        parts.append((np.full(30, sources[kind]), rng.integers(0, core, 30)))
    src = np.concatenate([s for s, _ in parts]).astype(np.int32)
    dst = np.concatenate([d for _, d in parts]).astype(np.int32)
    return Shape(V, src, dst, int(dst.max()) + 1, sources)


def records_of_levels(V, src, dst, levels):
    """the records of R.schedule (direction-optimising) read off finished levels: what the rule decides depends on F, M and the visited count only"""
    out_deg = np.bincount(src, minlength=V)
    factor = R.do_factor(V, len(src))
    reached = levels > 0
    F = np.bincount(levels[reached])[1:]
    M = np.bincount(levels[reached], weights=out_deg[reached]).astype(np.int64)[1:]
    records, prev_f, visited, bottom_up = [], 0, 0, False
    for lv, (f, m) in enumerate(zip(F, M), 1):
        f, m = int(f), int(m)
        visited += f
        if not bottom_up:
            bottom_up = R.turn_bottom_up(f, m, prev_f, visited, V, factor)
        elif R.turn_top_down(f, prev_f, visited, V, factor):
            bottom_up = False
        records.append(R.Level(lv, R.BOTTOM_UP if bottom_up else R.TOP_DOWN, f, m, None, None))
        prev_f = f
    return records


def small_m(V, env):
    """edge bound of the list kernel in direction-optimising mode (vgl_bfs_params_of: at most V / 15 - 1, off below 64)"""
    m = min(int(env.get("VGL_BFS_SMALL_M", 8192)), V // R.ALPHA - 1)
    return m if m >= 64 else 0


def scans_then_bottom_up(V, dst, records, env):
    """under `env` (VGL_TD_EMIT_EDGES=0 in it) some top-down level leaves its discoveries in `levels` only -- it has entries, more than the
    list kernel takes, and is not `late` (in_nz_rows + 1 - visited > V / 64) -- and the level after it, found by the scan, is bottom-up"""
    assert env.get("VGL_TD_EMIT_EDGES") == "0"
    in_nz, bound, visited = R.in_nz_rows(V, dst), small_m(V, env), 0
    for r, after in zip(records, records[1:]):
        visited += r.F
        late = max(0, in_nz + 1 - visited) <= V / 64
        if r.direction == R.TOP_DOWN and r.M > bound and not late and after.direction == R.BOTTOM_UP:
            return True
    return False


def scan_tiles(reach_rows, V):
    """vertex tiles the bounded scan launches"""
    return max(1, min(-(-V // TILE), -(-reach_rows // TILE)))
