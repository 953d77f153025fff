"""vgl_hip_bfs_run_batch with level offsets: between the first and the last traversal of a batch nothing re-initialises `levels` -- traversal k
stores o_k + level and takes every entry <= o_k for unvisited (o_0 = 0, o_(k+1) = o_k + the levels traversal k ran) -- and the last one runs at
offset 0 behind the fill of [0, reach_rows), so the buffer handed back holds plain levels.

Everything is judged by the restatement of tests/bfs_schedule_reference.py on its small inputs: the final levels are those of the batch's last
source, stats[i] those of source i, and the same batch under VGL_BFS_BATCH_REFILL=1 (a fill before every traversal, the behaviour before the
offsets) gives identical levels and identical statistics, `bu_edges` and `edges_examined` included.  A stale entry taken for visited would
show as a vertex not discovered (levels, `discovered`), one of this traversal's taken for unvisited as a frontier too large."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfs_schedule_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = ("VGL_BFS_SMALL_M", "VGL_BFS_BM_EXPAND", "VGL_TD_EMIT_EDGES", "VGL_BFS_NO_HINT", "VGL_TD_FILTER_SHARE", "VGL_TD_LATE_SHARE",
            "VGL_BFS_NO_SCAN_BOUND", "VGL_BFS_FILTER_F", "VGL_BFS_BLOCKED_SHARE", "VGL_BFS_BATCH_REFILL", "VGL_BFS_OFFSET_LIMIT")
ALL_STATS = ("levels", "edges_examined", "frontier_total", "discovered", "td_steps", "bu_steps", "td_edges", "td_frontier", "bu_edges", "bu_found",
             "algorithmic_bytes")
NUMBERINGS = (None, "total")
REFILL = {"VGL_BFS_BATCH_REFILL": "1"}
INT32_MAX = 2 ** 31 - 1


def modes():
    from vectorgraphlibrary_amd import api
    return (api.BFS_TOP_DOWN, api.BFS_DIRECTION_OPT)


class Case:
    """one input: the restatement per (source, mode) -- computed once, never written to -- and one graph handle per numbering"""

    def __init__(self, ctx, V, src, dst):
        self.ctx, self.V, self.src, self.dst = ctx, V, src, dst
        self.want, self.graphs = {}, {}

    def restated(self, source, mode):
        from vectorgraphlibrary_amd import api
        key = (int(source), mode)
        if key not in self.want:
            levels, records = R.schedule(self.V, self.src, self.dst, source, direction_optimising=mode == api.BFS_DIRECTION_OPT)
            levels.setflags(write=False)
            self.want[key] = (levels, R.expected(records), R.directions(records))
        return self.want[key]

    def graph(self, renumber=None):
        from vectorgraphlibrary_amd import api
        if renumber not in self.graphs:
            dev = lambda a: torch.from_numpy(a).to(self.ctx.device)
            self.graphs[renumber] = api.Graph.from_coo(self.ctx, self.V, dev(self.src), dev(self.dst), with_incoming=True, renumber=renumber)
        return self.graphs[renumber]

    def close(self):
        for g in self.graphs.values():
            g.close()
        self.graphs = {}


def batch(g, sources, mode, monkeypatch, env=None, levels=None):
    """api.bfs_batch from ORIGINAL source ids under `env`: (levels in the original numbering, levels in the graph's own, statistics)"""
    from vectorgraphlibrary_amd import api
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    try:
        raw, stats = api.bfs_batch(g, [g.vertex_id(s) for s in sources], mode, levels=levels)
        if levels is not None:
            assert raw.data_ptr() == levels.data_ptr()
        return g.to_original(raw).cpu().numpy(), raw.cpu().numpy(), stats
    finally:
        for name in env or {}:
            monkeypatch.delenv(name, raising=False)


def check_batch(case, g, sources, mode, monkeypatch, env=None, what=None, levels=None):
    """the batch against the restatement, and against itself with a fill before every traversal; returns the levels in the graph's numbering"""
    what = (what, tuple(sources), mode, env)
    lv, raw, stats = batch(g, sources, mode, monkeypatch, env, levels)
    assert np.array_equal(lv, case.restated(sources[-1], mode)[0]), what
    for i, (s, st) in enumerate(zip(sources, stats)):
        _, exp, directions = case.restated(s, mode)
        assert {k: st[k] for k in R.STATS} == exp, what + (i, directions)
        assert st["edges_examined"] == st["td_edges"] + st["bu_edges"], what + (i,)
    lv_refill, _, stats_refill = batch(g, sources, mode, monkeypatch, dict(env or {}, **REFILL))
    assert np.array_equal(lv, lv_refill), what
    assert [{k: st[k] for k in ALL_STATS} for st in stats] == [{k: st[k] for k in ALL_STATS} for st in stats_refill], what
    return raw


@pytest.fixture(scope="module")
def union(ctx):
    V, src, dst, sources = R.endings_union()
    case = Case(ctx, V, src, dst)
    yield case, sources
    case.close()


def union_batches(sources):
    """every ordered triple of the five endings as a batch of three (the middle traversal runs at an offset, after and before each ending), seeded
    draws of the orders of four and of five (two and three traversals at growing offsets), and one batch that repeats a source"""
    s = list(sources.values())
    assert len(s) == 5
    rng = np.random.default_rng(20)
    triples = list(itertools.permutations(s, 3))
    fours = list(itertools.permutations(s, 4))
    fives = list(itertools.permutations(s, 5))
    out = triples + [fours[i] for i in rng.choice(len(fours), 20, replace=False)] + [fives[i] for i in rng.choice(len(fives), 12, replace=False)]
    out.append((sources["bitmap_expand_finds_nothing"], sources["bitmap_expand_finds_nothing"], sources["bottom_up_finds_nothing"],
                sources["bitmap_expand_finds_nothing"], sources["bitmap_expand_finds_nothing"]))
    assert {t for b in out for t in zip(b, b[1:], b[2:])} >= set(triples)
    return [list(b) for b in out]


# ---- chained batches ----
@pytest.mark.parametrize("mode_index", [0, 1], ids=["top_down", "direction_optimising"])
@pytest.mark.parametrize("renumber", NUMBERINGS)
def test_chained_batches(union, monkeypatch, renumber, mode_index):
    case, sources = union
    g = case.graph(renumber)
    for b in union_batches(sources):
        check_batch(case, g, b, modes()[mode_index], monkeypatch, what=renumber)


# ---- every prefix ----
@pytest.mark.parametrize("renumber", NUMBERINGS)
def test_every_prefix_of_a_batch(union, monkeypatch, renumber):
    """whichever traversal happens to be the last one, no offset reaches the result"""
    case, sources = union
    g = case.graph(renumber)
    order = [sources[n] for n in ("bottom_up_finds_nothing", "list_kernel_finishes", "bitmap_expand_finds_nothing", "empty_count_after_top_down",
                                  "source_without_entries", "bitmap_expand_finds_nothing")]
    for mode in modes():
        for k in range(1, len(order) + 1):
            raw = check_batch(case, g, order[:k], mode, monkeypatch, what=(renumber, k))
            assert raw.min() == -1 and raw.max() == case.restated(order[k - 1], mode)[0].max(), (renumber, mode, k)


# ---- dirty buffer ----
def dirty(ctx, V, kind):
    if kind == "offsets":                                     # values that look like the entries a long batch leaves behind, and the extremes
        rng = np.random.default_rng(3)
        values = np.array([-1, 0, 1, 300, 4097, 1 << 20, 1 << 30, INT32_MAX - 1, INT32_MAX, -(1 << 31)], dtype=np.int64)
        return torch.from_numpy(rng.choice(values, V).astype(np.int32)).to(ctx.device)
    return torch.full((V,), kind, dtype=torch.int32, device=ctx.device)


@pytest.mark.parametrize("kind", [INT32_MAX, 12345, "offsets"], ids=["int32_max", "12345", "offsets"])
def test_dirty_buffer(ctx, union, monkeypatch, kind):
    case, sources = union
    order = [sources[n] for n in ("bitmap_expand_finds_nothing", "bottom_up_finds_nothing", "empty_count_after_top_down", "list_kernel_finishes")]
    for renumber in NUMBERINGS:
        g = case.graph(renumber)
        for mode in modes():
            for k in (1, 2, 3, 4):
                check_batch(case, g, order[:k], mode, monkeypatch, what=(renumber, kind, k), levels=dirty(ctx, case.V, kind))


# ---- every reader of "unvisited" ----
READER_ENVS = [{"VGL_TD_EMIT_EDGES": "0"},                                                    # non-emitting levels + vgl_k_bfs_scan_bound
               {"VGL_TD_EMIT_EDGES": "0", "VGL_BFS_NO_SCAN_BOUND": "1"},                     # the predicate of the count / write passes
               {"VGL_BFS_SMALL_M": "0"},
               {"VGL_BFS_SMALL_M": "0", "VGL_TD_EMIT_EDGES": "0"},
               {"VGL_TD_FILTER_SHARE": "0"}, {"VGL_TD_FILTER_SHARE": "2"},
               {"VGL_BFS_FILTER_F": "0"}, {"VGL_BFS_FILTER_F": str(1 << 30)}]
READER_SOURCES = {"two_bursts": [0, 8050 + 3, 8000 + 10, 0],                                 # first cluster, second cluster, the path between, again
                  "heavy_not_growing_shrunk": [0, 130, 5, 1]}                                # whole graph, second layer, first layer, whole graph but 0


@pytest.fixture(scope="module")
def reader_cases(ctx):
    made = {name: Case(ctx, *R.SHAPES[name]()[:3]) for name in READER_SOURCES}
    yield made
    for case in made.values():
        case.close()


@pytest.mark.parametrize("env", READER_ENVS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
@pytest.mark.parametrize("name", list(READER_SOURCES))
def test_every_reader_of_unvisited(reader_cases, monkeypatch, name, env):
    case = reader_cases[name]
    for renumber in NUMBERINGS:
        for mode in modes():
            check_batch(case, case.graph(renumber), READER_SOURCES[name], mode, monkeypatch, env, what=(name, renumber))


@pytest.mark.parametrize("name", list(READER_SOURCES))
def test_blocked_levels_in_a_batch(ctx, monkeypatch, name):
    """after prepare_blocked_bfs(), with VGL_BFS_BLOCKED_SHARE=0, the top-down levels of every traversal take the blocked pass"""
    case = Case(ctx, *R.SHAPES[name]()[:3])
    try:
        g = case.graph()
        g.prepare_blocked_bfs()
        for env in ({"VGL_BFS_BLOCKED_SHARE": "0"}, {"VGL_BFS_BLOCKED_SHARE": "0", "VGL_BFS_SMALL_M": "0"}):
            for mode in modes():
                check_batch(case, g, READER_SOURCES[name], mode, monkeypatch, env, what=name)
    finally:
        case.close()


# ---- deep levels and the overflow guard ----
def test_deep_levels_and_the_offset_limit(union, monkeypatch):
    """the path of 300 vertices (the component `list_kernel_finishes`), five traversals along it: the offsets are 300, 590, 890 and the last
    source's levels come back plain.  With VGL_BFS_OFFSET_LIMIT=500 the third traversal (offset 590) re-initialises and the offsets start again
    from its 300 levels; with 0 every traversal does.  The list kernel runs whole traversals here; with it off every level is a launch"""
    case, sources = union
    first = sources["list_kernel_finishes"]
    order = [first, first + 10, first, first + 150, first + 5]
    for mode in modes():
        assert [case.restated(s, mode)[1]["levels"] for s in order] == [300, 290, 300, 150, 295]
    for renumber in NUMBERINGS:
        g = case.graph(renumber)
        for mode in modes():
            for env in ({}, {"VGL_BFS_OFFSET_LIMIT": "500"}, {"VGL_BFS_OFFSET_LIMIT": "0"}, {"VGL_BFS_SMALL_M": "0", "VGL_BFS_OFFSET_LIMIT": "500"}):
                raw = check_batch(case, g, order, mode, monkeypatch, env, what=renumber)
                assert raw.max() == 295 and raw.min() == -1, (renumber, mode, env)


# ---- sources at or beyond reach_rows ----
def burst_with_spectators(extra=7):
    """R.burst and `extra` vertices without incoming entries, two outgoing entries each but the last, which has none: they are numbered last with
    and without the degree renumbering"""
    V, src, dst, _ = R.burst()
    rng = np.random.default_rng(11)
    new = np.arange(V, V + extra - 1)
    src = np.concatenate([src, np.repeat(new, 2)]).astype(np.int32)
    dst = np.concatenate([dst, rng.integers(0, V, 2 * len(new))]).astype(np.int32)
    assert (V + extra) % 64 != 0
    return V + extra, src, dst, V


@pytest.mark.parametrize("renumber", NUMBERINGS)
def test_sources_beyond_reach_rows(ctx, monkeypatch, renumber):
    V, src, dst, inner = burst_with_spectators()
    case = Case(ctx, V, src, dst)
    try:
        g = case.graph(renumber)
        reach = g.info()["reach_rows"]
        assert reach == inner
        x, y, lone = inner, inner + 3, V - 1
        a, b = 0, 17
        assert all(g.vertex_id(s) >= reach for s in (x, y, lone)) and all(g.vertex_id(s) < reach for s in (a, b))
        for order in ([x, a, b, a], [a, x, y, b], [a, b, a, x], [x, y, lone, x, a], [a, lone, lone, y], [x, x, x, x], [a, y, b, lone, a, x]):
            for mode in modes():
                raw = check_batch(case, g, order, mode, monkeypatch, what=renumber, levels=dirty(ctx, V, "offsets"))
                want_tail = np.full(V - reach, -1, np.int32)
                if g.vertex_id(order[-1]) >= reach:
                    want_tail[g.vertex_id(order[-1]) - reach] = 1
                assert np.array_equal(raw[reach:], want_tail), (renumber, order, mode)
    finally:
        case.close()


# ---- after a batch ----
def test_single_traversal_and_second_batch_after_a_batch(union, monkeypatch):
    from vectorgraphlibrary_amd import api
    case, sources = union
    s = list(sources.values())
    for renumber in NUMBERINGS:
        g = case.graph(renumber)
        for mode in modes():
            buf = torch.full((case.V,), 777, dtype=torch.int32, device=g.ctx.device)
            check_batch(case, g, s, mode, monkeypatch, what="first batch", levels=buf)
            for one in (s[2], s[0]):
                lv, st = api.bfs(g, one, mode, levels=buf)
                levels, exp, directions = case.restated(one, mode)
                assert np.array_equal(lv.cpu().numpy(), levels), (renumber, mode, one)
                assert {k: st[k] for k in R.STATS} == exp, (renumber, mode, one, directions)
            check_batch(case, g, s[::-1], mode, monkeypatch, what="second batch", levels=buf)
