"""reach_rows (1 + the largest vertex with an incoming entry; Graph.info()) and the two passes of the fused BFS that stop at it: the scan of
`levels` after a top-down level that did not emit (vgl_k_bfs_scan_bound over the vertex tiles below reach_rows) and the re-initialisation
between the traversals of a batch (vgl_hip_bfs_run_batch stores [0, reach_rows), the previous source and the new one).

The shapes come from tests/bfs_reach_rows_reference.py (renumber=None: the test controls the ids); tests/test_bfs_reach_rows_cpu.py asserts
without a GPU that every traversal used here reaches the scan and turns bottom-up after it.  Every traversal is compared with
oracle.bfs_top_down (all V levels), its statistics with the same traversal run alone through api.bfs into a fresh buffer, and the stand-alone
statistics with the restated schedule (tests/bfs_schedule_reference.py) -- a front bit of the source left behind beyond the scanned rows would
show there, as one vertex too many in the count that follows a scan."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfs_reach_rows_reference as RR  # noqa: E402
import bfs_schedule_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

STATS = ("levels", "edges_examined", "frontier_total", "discovered", "td_steps", "bu_steps", "bu_edges", "bu_found")
SWITCHES = ("VGL_TD_EMIT_EDGES", "VGL_BFS_SMALL_M", "VGL_BFS_NO_SCAN_BOUND")


def modes():
    from vectorgraphlibrary_amd import api
    return (api.BFS_TOP_DOWN, api.BFS_DIRECTION_OPT)


class Case:
    """one shape: its graph handle, the oracle's levels per source and the stand-alone traversals per (source, mode, env) -- each computed once"""

    def __init__(self, ctx, oracle, name):
        from vectorgraphlibrary_amd import api
        self.ctx, self.oracle, self.name, self.shape = ctx, oracle, name, RR.shape(name)
        s = self.shape
        dev = lambda a: torch.from_numpy(a).to(ctx.device)
        self.g = api.Graph.from_coo(ctx, s.V, dev(s.src), dev(s.dst), with_incoming=True, renumber=None)
        self.rowptr, self.adj = self.g.out_rowptr.cpu().numpy(), self.g.out_adj.cpu().numpy()
        self.refs, self.alone = {}, {}

    def ref(self, source):
        if source not in self.refs:
            levels = self.oracle.bfs_top_down(self.rowptr, self.adj, source)[0]
            levels.setflags(write=False)
            self.refs[source] = levels
        return self.refs[source]

    def stand_alone(self, source, mode, env, monkeypatch):
        """api.bfs into a fresh buffer: levels checked against the oracle, statistics against the restated schedule; returns the statistics"""
        from vectorgraphlibrary_amd import api
        key = (source, mode, tuple(sorted(env.items())))
        if key not in self.alone:
            with switches(monkeypatch, env):
                lv, st = api.bfs(self.g, source, mode, raw=True)
            what = (self.name,) + key
            assert np.array_equal(lv.cpu().numpy(), self.ref(source)), what
            s = self.shape
            records = R.schedule(s.V, s.src, s.dst, source, direction_optimising=mode == api.BFS_DIRECTION_OPT)[1]
            assert {k: st[k] for k in R.STATS} == R.expected(records), what + (R.directions(records),)
            self.alone[key] = {k: st[k] for k in STATS}
        return self.alone[key]

    def close(self):
        self.g.close()


class switches:
    def __init__(self, monkeypatch, env):
        self.mp, self.env = monkeypatch, env

    def __enter__(self):
        for name in SWITCHES:
            self.mp.delenv(name, raising=False)
        for name, value in self.env.items():
            self.mp.setenv(name, value)

    def __exit__(self, *exc):
        for name in self.env:
            self.mp.delenv(name, raising=False)


@pytest.fixture(scope="module")
def cases(ctx, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(ctx, oracle, name)
        return made[name]
    yield get
    for case in made.values():
        case.close()


def garbage(ctx, V, seed):
    """a levels buffer as a caller may hand it over: -1, 0, levels that a traversal could have left, large values"""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.choice(np.array([-1, 0, 1, 2, 3, 7, 12345], dtype=np.int32), V)).to(ctx.device)


# ---- reach_rows itself ----
@pytest.mark.parametrize("name", list(RR.LAYOUT))
def test_info_reports_reach_rows(cases, name):
    case = cases(name)
    assert case.g.info()["reach_rows"] == int(case.shape.dst.max()) + 1 == RR.LAYOUT[name][0]


def test_reach_rows_without_incoming_entries_and_without_incoming_csr(ctx):
    from vectorgraphlibrary_amd import api
    none = torch.zeros(0, dtype=torch.int32, device=ctx.device)
    g = api.Graph.from_coo(ctx, 777, none, none, with_incoming=True)
    try:
        assert g.info()["reach_rows"] == 0 and g.info()["in_nz_rows"] == 0
        for mode in modes():
            lv, st = api.bfs(g, 500, mode, levels=garbage(ctx, 777, 1))
            want = np.full(777, -1, np.int32)
            want[500] = 1
            assert np.array_equal(lv.cpu().numpy(), want) and st["discovered"] == 1
    finally:
        g.close()
    s = RR.shape("mid_byte")
    g = api.Graph.from_coo(ctx, s.V, torch.from_numpy(s.src).to(ctx.device), torch.from_numpy(s.dst).to(ctx.device), with_incoming=False)
    try:
        assert g.info()["reach_rows"] == s.V
    finally:
        g.close()


# ---- the bounded scan ----
@pytest.mark.parametrize("env", RR.SCAN_ENV, ids=["list_kernel", "no_list_kernel"])
@pytest.mark.parametrize("name", list(RR.LAYOUT))
def test_scan_below_reach_rows(ctx, cases, monkeypatch, name, env):
    """direction-optimising traversals whose level 3 (and, with the list kernel off, level 2) is found by the scan: from a source beyond the
    launched tiles (its front bit of the start must be gone after the scan, its visited bit kept), beyond reach_rows inside the last launched
    tile, inside the bound, and from an isolated vertex -- into a fresh buffer and, on the same handle, into one that holds garbage"""
    from vectorgraphlibrary_amd import api
    case = cases(name)
    for kind, source in case.shape.sources.items():
        alone = case.stand_alone(source, api.BFS_DIRECTION_OPT, env, monkeypatch)
        if kind != "isolated":
            assert alone["bu_steps"] > 0 and alone["td_steps"] >= 2, (name, kind)
        with switches(monkeypatch, env):
            lv, st = api.bfs(case.g, source, api.BFS_DIRECTION_OPT, levels=garbage(ctx, case.shape.V, source), raw=True)
        assert np.array_equal(lv.cpu().numpy(), case.ref(source)), (name, kind, env)
        assert {k: st[k] for k in STATS} == alone, (name, kind, env)


def test_scan_with_more_tiles_than_workgroups(ctx, oracle, monkeypatch):
    """2.2 M vertices, 1101 tiles below reach_rows (the scan has 1024 workgroups: some take two tiles per trip, the others one): levels against
    the oracle, statistics against the same traversal with the scan switched off (VGL_BFS_NO_SCAN_BOUND=1: the exact count reads all V levels)
    and against the directions the rule gives on the oracle's levels; then one batch over sources on both sides of the bound"""
    from vectorgraphlibrary_amd import api
    s = RR.many_tiles()
    g = api.Graph.from_coo(ctx, s.V, torch.from_numpy(s.src).to(ctx.device), torch.from_numpy(s.dst).to(ctx.device), with_incoming=True, renumber=None)
    try:
        assert g.info()["reach_rows"] == s.reach_rows and RR.scan_tiles(s.reach_rows, s.V) > RR.SCAN_BLOCKS
        rowptr, adj = g.out_rowptr.cpu().numpy(), g.out_adj.cpu().numpy()
        refs, alone = {}, {}
        for kind in ("far", "near", "inside"):
            source = s.sources[kind]
            refs[source] = oracle.bfs_top_down(rowptr, adj, source)[0]
            records = RR.records_of_levels(s.V, s.src, s.dst, refs[source])
            for env in RR.SCAN_ENV:
                assert RR.scans_then_bottom_up(s.V, s.dst, records, env), (kind, env)
                with switches(monkeypatch, env):
                    lv, st = api.bfs(g, source, api.BFS_DIRECTION_OPT, levels=garbage(ctx, s.V, source), raw=True)
                with switches(monkeypatch, dict(env, VGL_BFS_NO_SCAN_BOUND="1")):
                    lx, sx = api.bfs(g, source, api.BFS_DIRECTION_OPT, raw=True)
                assert np.array_equal(lv.cpu().numpy(), refs[source]) and np.array_equal(lx.cpu().numpy(), refs[source]), (kind, env)
                assert {k: st[k] for k in STATS} == {k: sx[k] for k in STATS}, (kind, env)
                assert st["levels"] == len(records) and st["frontier_total"] == sum(r.F for r in records), (kind, env)
                assert st["bu_steps"] == sum(r.direction == R.BOTTOM_UP for r in records) > 0, (kind, env)
                assert st["td_edges"] == sum(r.M for r in records if r.direction == R.TOP_DOWN), (kind, env)
                alone[source, tuple(env)] = {k: st[k] for k in STATS}
        refs[s.sources["far2"]] = oracle.bfs_top_down(rowptr, adj, s.sources["far2"])[0]
        order = [s.sources[k] for k in ("far", "far2", "inside", "far", "near")]
        for env in RR.SCAN_ENV:
            for n in (2, 3, 5):
                with switches(monkeypatch, env):
                    lv, stats = api.bfs_batch(g, order[:n], api.BFS_DIRECTION_OPT, levels=garbage(ctx, s.V, n))
                assert np.array_equal(lv.cpu().numpy(), refs[order[n - 1]]), (env, n)
                for src_i, st in zip(order[:n], stats):
                    if (src_i, tuple(env)) in alone:
                        assert {k: st[k] for k in STATS} == alone[src_i, tuple(env)], (env, n, src_i)
    finally:
        g.close()


# ---- the batch ----
def batch_sources(case):
    s = case.shape.sources
    if "far" not in s:
        return [s["inside"], s["inside"], 7]
    # two consecutive sources beyond reach_rows, the same source twice, beyond -> inside, inside -> beyond, an isolated source in the middle
    return [s["far"], s["far2"], s["far2"], s["inside"], s["far"], s["isolated"], s["near"], s["inside"]]


@pytest.mark.parametrize("env", [{}, RR.SCAN_ENV[1]], ids=["default", "scan"])
@pytest.mark.parametrize("name", ["mid_byte", "first_tile", "whole"])
def test_batch_reinitialises_what_a_traversal_can_have_written(ctx, cases, monkeypatch, name, env):
    """every prefix of the source list as one bfs_batch into a buffer of garbage: afterwards all V levels are those of a stand-alone traversal
    from the prefix's last source, and every traversal of the batch reports the statistics of its stand-alone run"""
    from vectorgraphlibrary_amd import api
    case = cases(name)
    sources = batch_sources(case)
    for mode in modes():
        alone = [case.stand_alone(s, mode, env, monkeypatch) for s in sources]
        for n in range(1, len(sources) + 1):
            buf = garbage(ctx, case.shape.V, 100 + n)
            with switches(monkeypatch, env):
                lv, stats = api.bfs_batch(case.g, sources[:n], mode, levels=buf)
            what = (name, mode, env, sources[:n])
            assert lv.data_ptr() == buf.data_ptr()
            assert np.array_equal(lv.cpu().numpy(), case.ref(sources[n - 1])), what
            assert [{k: st[k] for k in STATS} for st in stats] == alone[:n], what
