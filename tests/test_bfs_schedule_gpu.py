"""vgl_hip_bfs_run against the restated schedule (tests/bfs_schedule_reference.py): on every shaped input, in both modes, under every switch
setting, the levels AND the statistics the schedule fixes (levels, discovered, frontier_total, td_steps, bu_steps, td_frontier, td_edges, bu_found)
are the restatement's -- the direction of every level included, which no comparison of levels can see.  Which kernels ran is read off the launch
counts of the timing slots and compared with what the restatement says had to run (`check_witnesses`).

tests/test_bfs_schedule_cpu.py asserts, without a GPU, that every shape has the schedule it was built for."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfs_schedule_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = ("VGL_BFS_SMALL_M", "VGL_BFS_BM_EXPAND", "VGL_TD_EMIT_EDGES", "VGL_BFS_NO_HINT", "VGL_TD_FILTER_SHARE", "VGL_TD_LATE_SHARE",
            "VGL_BFS_NO_SCAN_BOUND", "VGL_BFS_FILTER_F", "VGL_BFS_BLOCKED_SHARE")
SLOTS = ("bfs_top_down", "bfs_bottom_up", "bfs_front_fold", "bfs_small_levels", "bfs_bitmap_expand", "bfs_blk_accumulate")
DEFAULT_FILTER_F = 65536
NUMBERINGS = (None, "total")


def _old(cap, bm, emit, nohint):
    names = ("VGL_BFS_SMALL_M", "VGL_BFS_BM_EXPAND", "VGL_TD_EMIT_EDGES", "VGL_BFS_NO_HINT")
    return {n: v for n, v in zip(names, (cap, bm, emit, nohint)) if v is not None}


# the twelve combinations of test_bfs_small_level_kernel_paths (tests/test_gpu_parity.py)
OLD_SETTINGS = [_old(*t) for t in (("0", None, None, None), (None, None, None, None), ("1000000", None, None, None), (None, "0", None, None),
                                   (None, "1000000000", None, None), ("256", "1000000000", None, None), (None, None, "0", None),
                                   (None, None, "1000000000000", None), ("0", "0", "0", None), (None, None, None, "1"),
                                   ("0", None, "1000000000000", "1"), ("1000000", "0", None, "1"))]
# the three switches no other test sets, each alone and with the list kernel off
NEW_SETTINGS = [dict(s, **extra) for s in ({"VGL_TD_FILTER_SHARE": "0"}, {"VGL_TD_FILTER_SHARE": "2"}, {"VGL_TD_LATE_SHARE": "0"},
                                           {"VGL_TD_LATE_SHARE": "1"}, {"VGL_BFS_NO_SCAN_BOUND": "1"})
                for extra in ({}, {"VGL_BFS_SMALL_M": "0"})]
PROBE_SETTINGS = [{"VGL_BFS_FILTER_F": "0"}, {"VGL_BFS_FILTER_F": str(1 << 30)}]      # these change the bottom-up probe (and so `bu_edges`)
assert len(OLD_SETTINGS) == 12 and len(NEW_SETTINGS) == 10


def modes():
    from vectorgraphlibrary_amd import api
    return (api.BFS_TOP_DOWN, api.BFS_DIRECTION_OPT)


class Case:
    """one input: its arrays, the restatement per (source, mode) -- computed once, never written to -- and graph handles per numbering"""

    def __init__(self, ctx, V, src, dst):
        self.ctx, self.V, self.src, self.dst = ctx, V, src, dst
        self.want, self.graphs = {}, {}

    def restated(self, source, mode):
        from vectorgraphlibrary_amd import api
        key = (int(source), mode)
        if key not in self.want:
            levels, records = R.schedule(self.V, self.src, self.dst, source, direction_optimising=mode == api.BFS_DIRECTION_OPT)
            levels.setflags(write=False)
            self.want[key] = (levels, tuple(records), R.expected(records))
        return self.want[key]

    def graph(self, renumber=None, **kw):
        from vectorgraphlibrary_amd import api
        if renumber not in self.graphs:
            dev = lambda a: torch.from_numpy(a).to(self.ctx.device)
            self.graphs[renumber] = api.Graph.from_coo(self.ctx, self.V, dev(self.src), dev(self.dst), with_incoming=True, renumber=renumber, **kw)
        return self.graphs[renumber]

    def close(self):
        for g in self.graphs.values():
            g.close()
        self.graphs = {}


@pytest.fixture(scope="module")
def cases(ctx):
    made = {}

    def get(name):
        if name not in made:
            V, src, dst, source = R.SHAPES[name]()
            made[name] = (Case(ctx, V, src, dst), source)
        return made[name]
    yield get
    for case, _ in made.values():
        case.close()


def traverse(ctx, g, source, mode, monkeypatch, env):
    """one api.bfs under `env` with the launches counted: (levels in the original numbering, statistics, launches per slot)"""
    from vectorgraphlibrary_amd import api
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    ctx.timing(True)
    try:
        lv, st = api.bfs(g, source, mode)
        launches = {slot: ctx.timing_get(slot)[0] for slot in SLOTS}
    finally:
        ctx.timing(False)
        for name in env:
            monkeypatch.delenv(name, raising=False)
    return lv.cpu().numpy(), st, launches


def check_stats(lv, st, want, what):
    levels, records, exp = want
    assert np.array_equal(lv, levels), what
    got = {k: st[k] for k in R.STATS}
    assert got == exp, (what, R.directions(records))
    assert st["edges_examined"] == st["td_edges"] + st["bu_edges"], what
    # every vertex a bottom-up level finds has been found by a probe that hit
    assert st["bu_edges"] >= st["bu_found"], what
    if exp["bu_steps"] == 0:
        assert st["bu_edges"] == 0, what


def check_witnesses(launches, records, env, what, blocked=False, list_kernel=True):
    """the launches the restated schedule demands under `env` (list_kernel: the graph is large enough for the list kernel's default edge bound,
    which direction-optimising mode caps at V / 15 - 1 and drops below 64)"""
    bu = [r for r in records if r.direction == R.BOTTOM_UP]
    td = [r for r in records if r.direction == R.TOP_DOWN]
    assert launches["bfs_bottom_up"] == len(bu), what
    filter_f = int(env.get("VGL_BFS_FILTER_F", DEFAULT_FILTER_F))
    assert launches["bfs_front_fold"] == sum(r.F <= filter_f for r in bu), what
    small_m = env.get("VGL_BFS_SMALL_M")
    if small_m == "0":
        assert launches["bfs_small_levels"] == 0 and launches["bfs_bitmap_expand"] == 0, what
        if not blocked:
            assert launches["bfs_top_down"] == sum(r.M > 0 for r in td), what
    elif small_m is None and list_kernel:
        assert launches["bfs_small_levels"] >= 1, what
    if env.get("VGL_BFS_BM_EXPAND") == "0":
        assert launches["bfs_bitmap_expand"] == 0, what
    if not blocked:
        assert launches["bfs_blk_accumulate"] == 0, what


def run_and_check(ctx, case, g, source, mode, monkeypatch, env, what, blocked=False):
    lv, st, launches = traverse(ctx, g, source, mode, monkeypatch, env)
    want = case.restated(source, mode)
    check_stats(lv, st, want, what)
    check_witnesses(launches, want[1], env, what, blocked)
    return st, launches


# ---- a. the schedule equals the restatement ----
@pytest.mark.parametrize("renumber", NUMBERINGS)
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_schedule_equals_restatement(ctx, cases, monkeypatch, name, renumber):
    case, source = cases(name)
    g = case.graph(renumber)
    assert g.info()["in_nz_rows"] == R.in_nz_rows(case.V, case.dst)
    for mode in modes():
        run_and_check(ctx, case, g, source, mode, monkeypatch, {}, (name, renumber, mode))


# ---- b. every switch setting ----
@pytest.mark.parametrize("renumber", NUMBERINGS)
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_every_switch_setting(ctx, cases, monkeypatch, name, renumber):
    case, source = cases(name)
    g = case.graph(renumber)
    for mode in modes():
        examined = {}
        for env in OLD_SETTINGS + NEW_SETTINGS + PROBE_SETTINGS:
            st, _ = run_and_check(ctx, case, g, source, mode, monkeypatch, env, (name, renumber, mode, env))
            if "VGL_BFS_FILTER_F" not in env:
                examined[tuple(sorted(env.items()))] = st["edges_examined"]
        assert len(set(examined.values())) == 1, (name, renumber, mode, examined)


# ---- c. path witnesses ----
def test_filter_bound_between_the_frontiers_of_a_phase(ctx, cases, monkeypatch):
    """two_bursts: each bottom-up phase has two levels with different F.  With VGL_BFS_FILTER_F between the two sizes exactly one level per phase
    folds its frontier: the F that bottom_up_level() sees is the level's own on every way in (a count launch that skipped on a hint or on the
    scan bound, staying bottom-up), not the previous level's"""
    from vectorgraphlibrary_amd import api
    case, source = cases("two_bursts")
    _, records, _ = case.restated(source, api.BFS_DIRECTION_OPT)
    ph = R.phases(records)
    assert len(ph) >= 2 and all(len(p) == 2 for p in ph)
    lo = max(min(p[0].F, p[1].F) for p in ph)
    hi = min(max(p[0].F, p[1].F) for p in ph)
    assert lo < hi, "one bound does not fit between the frontier sizes of every phase"
    bound = (lo + hi) // 2
    for renumber in NUMBERINGS:
        for extra in ({}, {"VGL_BFS_NO_HINT": "1"}, {"VGL_TD_EMIT_EDGES": "0"}, {"VGL_BFS_NO_SCAN_BOUND": "1", "VGL_TD_EMIT_EDGES": "0"},
                      {"VGL_BFS_SMALL_M": "0"}):
            env = dict(extra, VGL_BFS_FILTER_F=str(bound))
            _, launches = run_and_check(ctx, case, case.graph(renumber), source, api.BFS_DIRECTION_OPT, monkeypatch, env, (renumber, env))
            assert launches["bfs_front_fold"] == len(ph), (renumber, env)
    # all of them by default, none with the bound 0
    _, launches = run_and_check(ctx, case, case.graph(), source, api.BFS_DIRECTION_OPT, monkeypatch, {}, "default")
    assert launches["bfs_front_fold"] == sum(len(p) for p in ph) and launches["bfs_bitmap_expand"] >= 2
    _, launches = run_and_check(ctx, case, case.graph(), source, api.BFS_DIRECTION_OPT, monkeypatch, {"VGL_BFS_FILTER_F": "0"}, "never")
    assert launches["bfs_front_fold"] == 0


def test_ids_hand_over_into_a_bottom_up_level(ctx, cases, monkeypatch):
    """hub_layer: level 2 is 40 vertices with 60 000 entries -- the list kernel leaves with its list as `ids` and the level turns bottom-up at
    once; with the bound at 40 that level folds, with 39 it does not"""
    from vectorgraphlibrary_amd import api
    case, source = cases("hub_layer")
    _, records, _ = case.restated(source, api.BFS_DIRECTION_OPT)
    first = records[1]
    assert first.direction == R.BOTTOM_UP and all(r.F > first.F for r in records[2:] if r.direction == R.BOTTOM_UP)
    for bound, folds in ((first.F, 1), (first.F - 1, 0)):
        _, launches = run_and_check(ctx, case, case.graph(), source, api.BFS_DIRECTION_OPT, monkeypatch, {"VGL_BFS_FILTER_F": str(bound)}, bound)
        assert launches["bfs_front_fold"] == folds and launches["bfs_small_levels"] >= 1


@pytest.mark.parametrize("name", ["two_bursts", "heavy_not_growing_shrunk"])
def test_blocked_levels(ctx, monkeypatch, name):
    """after prepare_blocked_bfs(), with VGL_BFS_BLOCKED_SHARE=0 and the list kernel off, every top-down level takes the blocked pass"""
    from vectorgraphlibrary_amd import api
    V, src, dst, source = R.SHAPES[name]()
    case = Case(ctx, V, src, dst)
    try:
        g = case.graph()
        plain, _ = run_and_check(ctx, case, g, source, api.BFS_TOP_DOWN, monkeypatch, {"VGL_BFS_SMALL_M": "0"}, "before")
        g.prepare_blocked_bfs()
        env = {"VGL_BFS_BLOCKED_SHARE": "0", "VGL_BFS_SMALL_M": "0"}
        st, launches = run_and_check(ctx, case, g, source, api.BFS_TOP_DOWN, monkeypatch, env, "blocked", blocked=True)
        assert launches["bfs_top_down"] == 0 and launches["bfs_blk_accumulate"] > 0
        assert {k: st[k] for k in R.STATS + ("edges_examined",)} == {k: plain[k] for k in R.STATS + ("edges_examined",)}
        # direction-optimising, default share: blocked or not, the schedule is the restatement's
        run_and_check(ctx, case, g, source, api.BFS_DIRECTION_OPT, monkeypatch, {}, "prepared, direction-optimising", blocked=True)
    finally:
        case.close()


# ---- d. chained traversals on one handle ----
@pytest.fixture(scope="module")
def union(ctx):
    V, src, dst, sources = R.endings_union()
    case = Case(ctx, V, src, dst)
    yield case, sources
    case.close()


def test_union_traversals_end_in_every_way(ctx, union, monkeypatch):
    """which component of R.ENDINGS gives which ending, read off the launch counts (default switches, direction-optimising mode)"""
    from vectorgraphlibrary_amd import api
    case, sources = union
    g = case.graph()
    got = {}
    for name, s in sources.items():
        _, got[name] = run_and_check(ctx, case, g, s, api.BFS_DIRECTION_OPT, monkeypatch, {}, name)
    rec = {name: case.restated(s, api.BFS_DIRECTION_OPT)[1] for name, s in sources.items()}
    # a path of 300: nothing but the list kernel expands a level, so it is the list kernel that meets the empty frontier
    n = got["list_kernel_finishes"]
    assert n["bfs_small_levels"] >= 1 and n["bfs_top_down"] == 0 and n["bfs_bottom_up"] == 0 and n["bfs_bitmap_expand"] == 0
    # one cluster: after the bottom-up phase the last level (discovers nothing) is expanded from the bitmap: the only expand launch, and the only
    # list kernel launch besides the one from the source
    n, r = got["bitmap_expand_finds_nothing"], rec["bitmap_expand_finds_nothing"]
    assert r[-2].direction == R.BOTTOM_UP and r[-1].found == 0
    assert n["bfs_bitmap_expand"] == 1 and n["bfs_small_levels"] == 2 and n["bfs_bottom_up"] == len(R.phases(r)[0])
    # closed heavy layers: every level the list kernel cannot take is one bfs_top_down launch, the last one (discovers nothing) included; the list
    # kernel runs once, from the source
    n, r = got["empty_count_after_top_down"], rec["empty_count_after_top_down"]
    small_m = min(8192, case.V // 15 - 1)
    assert r[-1].found == 0 and r[-1].M > small_m
    assert n["bfs_small_levels"] == 1 and n["bfs_bitmap_expand"] == 0 and n["bfs_bottom_up"] == 0
    assert n["bfs_top_down"] == sum(x.M > small_m for x in r)
    # the hub: bottom-up from the first level, the last bottom-up level finds nothing
    n, r = got["bottom_up_finds_nothing"], rec["bottom_up_finds_nothing"]
    assert n["bfs_bottom_up"] == len(r) and n["bfs_top_down"] == 0 and n["bfs_bitmap_expand"] == 0 and n["bfs_small_levels"] == 1
    # a vertex without entries: the list kernel ends it; with the list kernel off it is a level that launches no expansion and an empty count
    n = got["source_without_entries"]
    assert n == dict(n, bfs_small_levels=1, bfs_top_down=0, bfs_bottom_up=0, bfs_bitmap_expand=0)
    _, n = run_and_check(ctx, case, g, sources["source_without_entries"], api.BFS_DIRECTION_OPT, monkeypatch, {"VGL_BFS_SMALL_M": "0"}, "no entries")
    assert n == dict(n, bfs_small_levels=0, bfs_top_down=0, bfs_bottom_up=0, bfs_bitmap_expand=0)


@pytest.mark.parametrize("env", [{}, {"VGL_BFS_SMALL_M": "0"}], ids=["default", "no_list_kernel"])
def test_chained_traversals_on_one_handle(ctx, union, monkeypatch, env):
    """every ordered pair (a traversal ending one way, then another traversal) on the same handle: the second one has the restated schedule,
    run singly and as the second of a bfs_batch -- whatever the first left in the counters, the bitmaps and the hint does not reach it"""
    from vectorgraphlibrary_amd import api
    case, sources = union
    g = case.graph()
    for mode in modes():
        for first, x in sources.items():
            for second, y in sources.items():
                what = (first, second, mode)
                traverse(ctx, g, x, mode, monkeypatch, env)
                lv, st, launches = traverse(ctx, g, y, mode, monkeypatch, env)
                want = case.restated(y, mode)
                check_stats(lv, st, want, what)
                check_witnesses(launches, want[1], env, what)
                for name, value in env.items():
                    monkeypatch.setenv(name, value)
                lv, stats = api.bfs_batch(g, [x, y], mode)
                for name in env:
                    monkeypatch.delenv(name)
                check_stats(lv.cpu().numpy(), stats[1], want, what + ("batch",))
                check_stats(case.restated(x, mode)[0], stats[0], case.restated(x, mode), what + ("batch, first",))
    # the direction-optimising traversal after a top-down one and the other way round
    td, do = modes()
    for x in sources.values():
        for y in sources.values():
            traverse(ctx, g, x, td, monkeypatch, env)
            lv, st, _ = traverse(ctx, g, y, do, monkeypatch, env)
            check_stats(lv, st, case.restated(y, do), (x, y, "top-down first"))
            lv, st, _ = traverse(ctx, g, x, td, monkeypatch, env)
            check_stats(lv, st, case.restated(x, td), (x, y, "direction-optimising first"))
    # the first traversal under the default switches, the second under `env`: with the list kernel on, the last launch that left a frontier size
    # and an edge count on the device is a real switch to bottom-up (the chain of test_bfs_level_without_edges_leaves_no_stale_direction_hint)
    for x in sources.values() if env else ():
        for y in sources.values():
            traverse(ctx, g, x, do, monkeypatch, {})
            lv, st, launches = traverse(ctx, g, y, do, monkeypatch, env)
            check_stats(lv, st, case.restated(y, do), (x, y, "default switches first"))
            check_witnesses(launches, case.restated(y, do)[1], env, (x, y, "default switches first"))


# ---- e. bounded fuzz ----
@pytest.mark.parametrize("seed", range(12))
def test_fuzz_against_oracle_and_restatement(ctx, oracle, monkeypatch, seed):
    """the generator of tests/studies/fuzz_bfs.py with V <= 2^15 (every fifth seed with its glued-on path), the switches drawn at random: levels
    against the oracle, statistics against the restatement"""
    from vectorgraphlibrary_amd import api
    V, src, dst, rng = R.study_graph(seed, log_v_end=16)
    case = Case(ctx, V, src, dst)
    rowptr, adj, _ = oracle.coo_to_csr(V, src, dst)
    try:
        g = case.graph([None, "total", "out", "in"][seed % 4])
        for source in sorted({int(rng.integers(0, V)), int(np.argmax(np.diff(rowptr))), 0}):
            ref = oracle.bfs_top_down(rowptr, adj, source)[0]
            for mode in modes():
                examined = set()
                for k in range(3):
                    env = {}
                    if k:
                        env["VGL_BFS_SMALL_M"] = str(int(rng.choice([0, 64, 300, 8192, 1000000])))
                        env["VGL_BFS_BM_EXPAND"] = str(int(rng.choice([0, 100, 262144, 1 << 30])))
                        for name, values in (("VGL_BFS_NO_HINT", ["1"]), ("VGL_TD_EMIT_EDGES", ["0", "4096", str(1 << 40)]),
                                             ("VGL_BFS_NO_SCAN_BOUND", ["1"]), ("VGL_TD_FILTER_SHARE", ["0", "0.5", "2"]),
                                             ("VGL_TD_LATE_SHARE", ["0", "0.25", "1"])):
                            if rng.random() < 0.5:
                                env[name] = str(rng.choice(values))
                    what = (seed, source, mode, env)
                    lv, st, launches = traverse(ctx, g, source, mode, monkeypatch, env)
                    assert np.array_equal(lv, ref), what
                    want = case.restated(source, mode)
                    check_stats(lv, st, want, what)
                    check_witnesses(launches, want[1], env, what, list_kernel=V >= 1024)
                    examined.add(st["edges_examined"])
                assert len(examined) == 1, (seed, source, mode, examined)
    finally:
        case.close()


# ---- f. refusal ----
def test_direction_optimising_without_incoming_csr_is_refused(ctx):
    from vectorgraphlibrary_amd import api
    from vectorgraphlibrary_amd.lib import VglHipError
    V, src, dst, source = R.burst(n=1000)
    g = api.Graph.from_coo(ctx, V, torch.from_numpy(src).to(ctx.device), torch.from_numpy(dst).to(ctx.device), with_incoming=False)
    try:
        levels = torch.full((V,), 12345, dtype=torch.int32, device=ctx.device)
        with pytest.raises(VglHipError, match="incoming CSR"):
            api.bfs(g, source, api.BFS_DIRECTION_OPT, levels=levels)
        assert bool((levels == 12345).all())
        lv, _ = api.bfs(g, source, api.BFS_TOP_DOWN, levels=levels)              # top-down mode does not need it
        assert np.array_equal(lv.cpu().numpy(), R.schedule(V, src, dst, source, direction_optimising=False)[0])
    finally:
        g.close()
