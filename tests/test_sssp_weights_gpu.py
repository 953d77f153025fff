"""Every shortest-path / widest-path schedule of the HIP library on ADVERSARIAL edge weights (run with -m gpu on a MI355X): zeros and zero-weight
cycles, mass ties, weights on the light / heavy boundary of the delta plan, degenerate (all-light, all-heavy) plans, extreme deltas, denormal and
tiny weights, a dynamic range of 200 binades, and capacities 0 / all equal / FLT_MAX.  The references are the oracle's Bellman-Ford runs, which
tests/test_sssp_weights_cpu.py ties to two independent computations; the fixed point is unique on this domain (sssp_weights_reference.py), so
every comparison is on the int32 views of the float32 results."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import sssp_weights_reference as R

pytestmark = pytest.mark.gpu

MAIN = ["rmat_s12_e16", "ru_s13_e8", "ring_300"]
SMALL = ["ring_1024", "rmat_s10_e8"]
# the delta variants of a class that are left out because they are not positive: "zeros" has no positive weight
OMITTED_DELTAS = {("zeros", "max"), ("zeros", "min_positive")}

_BUILT = {}      # graph name -> device graph + host CSR + source + BFS levels
_REFS = {}       # (graph name, "sssp" | "sswp", class) -> (device values in CSR order, host values in CSR order, oracle result)


@pytest.fixture(scope="module", autouse=True)
def _release_graphs():
    yield
    for c in _BUILT.values():
        c.g.close()
    _BUILT.clear()
    _REFS.clear()


def _graph_dict(O, name):
    for g in R.graphs(O) + R.small_graphs(O) + [R.block_pair_graph(O)]:
        if g["name"] == name:
            return g
    raise KeyError(name)


def case(ctx, O, name):
    if name not in _BUILT:
        import torch
        from vectorgraphlibrary_amd import api
        gd = _graph_dict(O, name)
        src_d, dst_d = torch.from_numpy(gd["src"]).to(ctx.device), torch.from_numpy(gd["dst"]).to(ctx.device)
        g = api.Graph.from_coo(ctx, gd["V"], src_d, dst_d, want_perm=True)
        rowptr, adj, perm = O.coo_to_csr(gd["V"], gd["src"], gd["dst"])
        assert (g.out_rowptr.cpu().numpy() == rowptr).all() and (g.out_adj.cpu().numpy() == adj).all() and (g.perm.cpu().numpy() == perm).all()
        source = O.pick_source(rowptr, gd["seed"])
        levels, _ = O.bfs_top_down(rowptr, adj, source)
        _BUILT[name] = SimpleNamespace(name=name, g=g, V=gd["V"], E=len(gd["src"]), seed=gd["seed"], rowptr=rowptr, adj=adj, perm=perm, source=source,
                                       levels=levels)
    return _BUILT[name]


def values(ctx, O, c, kind, cls):
    """(device values in CSR order, the same on the host, the oracle's result from c.source), computed once"""
    key = (c.name, kind, cls)
    if key not in _REFS:
        import torch
        w_in = R.make(R.WEIGHT_CLASSES if kind == "sssp" else R.CAPACITY_CLASSES, cls, c.E, c.seed)
        w = w_in[c.perm]
        w_d = ctx.gather_u32(c.g.perm, torch.from_numpy(w_in).to(ctx.device))
        assert (w_d.cpu().numpy().view(np.int32) == w.view(np.int32)).all()          # denormals and zeros arrive on the device as they are
        ref = (O.sssp_bellman_ford if kind == "sssp" else O.sswp_bellman_ford)(c.rowptr, c.adj, w, c.source)[0]
        ref.setflags(write=False)
        _REFS[key] = (w_d, w, ref)
    return _REFS[key]


def bits(t):
    return t.cpu().numpy().view(np.int32)


def same(t, ref, what):
    got = bits(t)
    bad = np.flatnonzero(got != ref.view(np.int32))
    assert bad.size == 0, "%s: %d of %d values differ from the oracle, first at vertex %d: %r vs %r" % (
        what, bad.size, got.size, bad[0], got.view(np.float32)[bad[0]], ref[bad[0]])


def delta_variants(cls, w):
    """the four deltas of the issue: 16, max(w) (only the maximum is heavy), the smallest positive w (every positive edge heavy) and
    2 max(w) + 1 (every edge light); the ones that are not positive are the OMITTED_DELTAS"""
    pos = w[w > 0]
    out = [("16", 16.0), ("all_light", float(np.float32(2.0) * w.max() + np.float32(1.0)))]
    if pos.size:
        out += [("max", float(w.max())), ("min_positive", float(pos.min()))]
    assert {(cls, n) for n in ("16", "all_light", "max", "min_positive")} - {(cls, n) for n, _ in out} == {k for k in OMITTED_DELTAS if k[0] == cls}
    assert all(d > 0 and np.isfinite(d) for _, d in out)
    return out


def check_stats(api, mode, st):
    assert st["push_steps"] + st["pull_steps"] == st["iterations"]
    if mode == api.SSSP_PULL:
        assert st["push_steps"] == 0


def run_all_sssp(api, monkeypatch, c, w_d, w, cls):
    """[(label, distances)] of every schedule: the four modes of vgl_hip_sssp_run (ALL_ACTIVE both as blocked passes and as the atomic push kernel:
    the graph carries the path structure after the first PULL) and delta-stepping with the four deltas"""
    out = []
    for mode in (api.SSSP_PULL, api.SSSP_DIRECTION_OPT, api.SSSP_ACTIVE_TILES, api.SSSP_ALL_ACTIVE):
        d, st = api.sssp(c.g, w_d, c.source, mode)
        check_stats(api, mode, st)
        out.append(("mode %d" % mode, d))
    with monkeypatch.context() as m:
        m.setenv("VGL_SSSP_ALL_ACTIVE_PUSH", "1")
        d, st = api.sssp(c.g, w_d, c.source, api.SSSP_ALL_ACTIVE)
        assert st["pull_steps"] == 0 and st["push_steps"] == st["iterations"]
        out.append(("mode 0 (atomic push)", d))
    for name, delta in delta_variants(cls, w):
        d, st = api.sssp(c.g, w_d, c.source, api.SSSP_DELTA_STEPPING, delta=delta)
        out.append(("delta-stepping, delta = %s (%r)" % (name, delta), d))
    return out


def run_all_sswp(api, monkeypatch, c, cap_d):
    out = []
    for mode in (api.SSSP_PULL, api.SSSP_DIRECTION_OPT, api.SSSP_ACTIVE_TILES, api.SSSP_ALL_ACTIVE):
        wd, st = api.sswp(c.g, cap_d, c.source, mode)
        check_stats(api, mode, st)
        out.append(("mode %d" % mode, wd))
    with monkeypatch.context() as m:
        m.setenv("VGL_SSSP_ALL_ACTIVE_PUSH", "1")
        wd, st = api.sswp(c.g, cap_d, c.source, api.SSSP_ALL_ACTIVE)
        assert st["pull_steps"] == 0
        out.append(("mode 0 (atomic push)", wd))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# a. every class x every schedule
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", MAIN)
@pytest.mark.parametrize("cls", sorted(R.WEIGHT_CLASSES))
def test_sssp_every_schedule_on_every_weight_class(cls, gname, ctx, oracle, monkeypatch):
    from vectorgraphlibrary_amd import api
    c = case(ctx, oracle, gname)
    w_d, w, ref = values(ctx, oracle, c, "sssp", cls)
    reached = c.levels > 0
    assert reached.mean() >= 0.5 and ((ref < R.FLT_MAX) == reached).all()
    if cls == "ones":
        assert (ref[reached] == (c.levels[reached] - 1).astype(np.float32)).all()      # the independent cross-check: BFS levels (they start at 1)
    t0 = time.perf_counter()
    for label, d in run_all_sssp(api, monkeypatch, c, w_d, w, cls):
        same(d, ref, "SSSP %s on %s, %s" % (cls, gname, label))
    print("sssp %s %s: %.2f s" % (cls, gname, time.perf_counter() - t0))


@pytest.mark.parametrize("gname", MAIN)
@pytest.mark.parametrize("cls", sorted(R.CAPACITY_CLASSES))
def test_sswp_every_schedule_on_every_capacity_class(cls, gname, ctx, oracle, monkeypatch):
    from vectorgraphlibrary_amd import api
    c = case(ctx, oracle, gname)
    cap_d, cap, ref = values(ctx, oracle, c, "sswp", cls)
    for label, wd in run_all_sswp(api, monkeypatch, c, cap_d):
        same(wd, ref, "SSWP %s on %s, %s" % (cls, gname, label))
        wv = wd.cpu().numpy()
        assert wv[c.source] == R.FLT_MAX and (wv[c.levels < 0] == 0).all()
        if cls == "zeros":
            assert (wv[np.arange(c.V) != c.source] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# b. boundary deltas
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", MAIN)
def test_delta_on_the_light_heavy_boundary(gname, ctx, oracle):
    """weights 16 and nextafter(16, 0): delta = nextafter(16, 0) makes every edge heavy, 16 splits the two values, nextafter(16, inf) makes every
    edge light -- three different plans, one result"""
    from vectorgraphlibrary_amd import api
    c = case(ctx, oracle, gname)
    w_d, w, ref = values(ctx, oracle, c, "sssp", "two_values")
    lo, hi = np.nextafter(np.float32(16.0), np.float32(0.0)), np.nextafter(np.float32(16.0), np.float32(np.inf))
    assert set(np.unique(w)) == {lo, np.float32(16.0)}
    deltas = (16.0, float(lo), float(hi))
    n_light = sorted(int((w < np.float32(x)).sum()) for x in deltas)
    assert n_light[0] == 0 < n_light[1] < n_light[2] == c.E                            # all heavy, split, all light
    for delta in deltas:
        d, _ = api.sssp(c.g, w_d, c.source, api.SSSP_DELTA_STEPPING, delta=delta)
        same(d, ref, "two_values on %s, delta %r" % (gname, delta))
        plan = api.SsspPlan(c.g, w_d, delta)                                           # ... and as a reusable plan
        d, _ = api.sssp(c.g, None, c.source, plan=plan)
        plan.close()
        same(d, ref, "two_values on %s, plan with delta %r" % (gname, delta))


@pytest.mark.parametrize("gname", SMALL)
@pytest.mark.parametrize("cls", ["sparse_zeros", "top_of_domain"])
@pytest.mark.parametrize("delta", [float("inf"), 2.0 ** -149], ids=["inf", "denormal"])
def test_extreme_deltas_are_accepted(delta, cls, gname, ctx, oracle):
    """the documented behaviour (include/vgl_hip.h): delta = +inf is one bucket with every edge light, the smallest denormal makes a bucket of every
    distinct distance with every positive edge heavy; both end at the fixed point"""
    from vectorgraphlibrary_amd import api
    c = case(ctx, oracle, gname)
    w_d, w, ref = values(ctx, oracle, c, "sssp", cls)
    t0 = time.perf_counter()
    d, st = api.sssp(c.g, w_d, c.source, api.SSSP_DELTA_STEPPING, delta=delta)
    print("delta %r %s %s: %d steps, %.2f s" % (delta, cls, gname, st["iterations"], time.perf_counter() - t0))
    same(d, ref, "%s on %s, delta %r" % (cls, gname, delta))


@pytest.mark.parametrize("delta", [0.0, -1.0, float("nan"), float("-inf")], ids=["zero", "negative", "nan", "minus_inf"])
def test_non_positive_deltas_are_refused(delta, ctx, oracle):
    import torch
    from vectorgraphlibrary_amd import api, lib
    c = case(ctx, oracle, "ring_300")
    w_d, w, ref = values(ctx, oracle, c, "sssp", "ones")
    dist = torch.full((c.V,), 7.0, dtype=torch.float32, device=ctx.device)
    with pytest.raises(lib.VglHipError, match="delta must be positive"):
        api.sssp(c.g, w_d, c.source, api.SSSP_DELTA_STEPPING, dist=dist, delta=delta)
    with pytest.raises(lib.VglHipError, match="delta must be positive"):
        api.SsspPlan(c.g, w_d, delta)
    assert bool((dist == 7.0).all()), "a refused call wrote to dist"
    d, _ = api.sssp(c.g, w_d, c.source, api.SSSP_DELTA_STEPPING, delta=16.0)           # the handle is as usable as before
    same(d, ref, "after the refusals")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# c. forced paths on a graph with a block pair
# ---------------------------------------------------------------------------------------------------------------------------------------------
# a delta that leaves both parts of the plan non-empty (for small_ints it EQUALS a weight) and keeps the number of buckets small
FORCED_DELTA = {"sparse_zeros": 16.0, "small_ints": 2.0, "denormals": 2.0 ** -130, "wide_range": 2.0 ** 40}


@pytest.mark.parametrize("cls", sorted(FORCED_DELTA))
def test_forced_delta_stepping_paths(cls, ctx, oracle, monkeypatch):
    """the three frontier selections of a delta-stepping step and its dense steps as blocked passes (heavy part / both parts, with and without
    fused tiles), each forced"""
    from vectorgraphlibrary_amd import api
    c = case(ctx, oracle, "rmat_s15_e16")
    w_d, w, ref = values(ctx, oracle, c, "sssp", cls)
    delta = FORCED_DELTA[cls]
    n_light = int((w < np.float32(delta)).sum())
    assert 0 < n_light < c.E
    t0 = time.perf_counter()
    for wide, small in (("1", "4096"), ("0", "0"), ("0", "1000000000")):
        with monkeypatch.context() as m:
            m.setenv("VGL_DS_WIDE", wide), m.setenv("VGL_DS_SMALL", small)
            d, _ = api.sssp(c.g, w_d, c.source, api.SSSP_DELTA_STEPPING, delta=delta)
        same(d, ref, "%s, VGL_DS_WIDE=%s VGL_DS_SMALL=%s" % (cls, wide, small))
    # that the switch was honoured shows in the context's launch counts: a plan loads its values into one blocked layout per blocked part
    # (one piece each at this size) and into none without the switch; a part that has a layout takes the blocked pass in every dense step,
    # and with a dense share of 0 every heavy step is dense
    def layouts_loaded(env):
        ctx.timing(True, only="blk_load_weights")
        try:
            with monkeypatch.context() as m:
                for k, v in env.items():
                    m.setenv(k, v)
                d, st = api.sssp(c.g, w_d, c.source, api.SSSP_DELTA_STEPPING, delta=delta)
            return d, st, ctx.timing_get("blk_load_weights")[0]
        finally:
            ctx.timing(False)
    d, st, n = layouts_loaded({})
    assert n == 0 and st["iterations"] > 0
    for blocked in ("1", "2"):
        for fuse in ("0", "64"):
            d, st, n = layouts_loaded({"VGL_DS_BLOCKED": blocked, "VGL_BLK_FUSE_MIN": fuse, "VGL_DS_DENSE": "0", "VGL_DS_DENSE_BLK": "0"})
            assert n == int(blocked), "VGL_DS_BLOCKED=%s: values were loaded into %d blocked layouts" % (blocked, n)
            same(d, ref, "%s, VGL_DS_BLOCKED=%s VGL_BLK_FUSE_MIN=%s" % (cls, blocked, fuse))
    print("forced delta-stepping %s: %.2f s" % (cls, time.perf_counter() - t0))


@pytest.mark.parametrize("cls", sorted(FORCED_DELTA))
def test_forced_pull_layouts_and_switch_points(cls, ctx, oracle, monkeypatch):
    """pull plans in three forced layouts (blocks cut into 64-chunk units, block pairs as fused tiles, row-range pieces), SSSP and SSWP through the
    same plan, pull only and push <-> pull at three switch points"""
    from vectorgraphlibrary_amd import api
    c = case(ctx, oracle, "rmat_s15_e16")
    w_d, w, ref = values(ctx, oracle, c, "sssp", cls)
    refw, _ = oracle.sswp_bellman_ford(c.rowptr, c.adj, w, c.source)
    t0 = time.perf_counter()
    layouts = ({"VGL_BLK_GATHER_UNIT": "64", "VGL_BLK_ACCUM_UNIT": "64", "VGL_BLK_FUSED_UNIT": "64"}, {"VGL_BLK_FUSE_MIN": "64"},
               {"VGL_BLK_PIECE_EDGES": str(c.E // 7)})
    for layout in layouts:
        with monkeypatch.context() as m:
            for k, v in layout.items():
                m.setenv(k, v)
            plan = api.SsspPullPlan(c.g, w_d)
        info = plan.info()
        assert info["edges"] == c.E
        if "VGL_BLK_FUSE_MIN" in layout:
            assert info["fused_edges"] > 0
        for share in ("0", "0.35", "2"):
            with monkeypatch.context() as m:
                m.setenv("VGL_SSSP_PULL_SHARE", share)
                d, st = api.sssp(c.g, w_d, c.source, api.SSSP_DIRECTION_OPT, plan=plan)
                wd, wst = api.sswp(c.g, w_d, c.source, api.SSSP_DIRECTION_OPT, plan=plan)
            same(d, ref, "SSSP %s, layout %r, share %s" % (cls, layout, share))
            same(wd, refw, "SSWP %s, layout %r, share %s" % (cls, layout, share))
            for s in (st, wst):
                assert s["push_steps"] + s["pull_steps"] == s["iterations"]
                if share == "2":
                    assert s["pull_steps"] == 0
        d, st = api.sssp(c.g, w_d, c.source, api.SSSP_PULL, plan=plan)
        wd, wst = api.sswp(c.g, w_d, c.source, api.SSSP_PULL, plan=plan)
        same(d, ref, "SSSP %s, layout %r, pull" % (cls, layout))
        same(wd, refw, "SSWP %s, layout %r, pull" % (cls, layout))
        assert st["push_steps"] == 0 and wst["push_steps"] == 0
        plan.close()
    print("forced pull layouts %s: %.2f s" % (cls, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# d. plan reuse across weight classes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_plans_of_two_weight_classes_on_one_handle_stay_apart(ctx, oracle):
    """the path structure is per graph, the value arrays per weights: plans built from all-zero weights and from wide_range weights, sources
    interleaved between them -- a value array left over from the other plan would show at once"""
    from vectorgraphlibrary_amd import api
    O = oracle
    c = case(ctx, O, "rmat_s12_e16")
    (z_d, z, _), (r_d, r, _) = values(ctx, O, c, "sssp", "zeros"), values(ctx, O, c, "sssp", "wide_range")
    c.g.prepare_sssp()
    pull = {"zeros": api.SsspPullPlan(c.g, z_d), "wide_range": api.SsspPullPlan(c.g, r_d)}
    bucketed = {"zeros": api.SsspPlan(c.g, z_d, 16.0), "wide_range": api.SsspPlan(c.g, r_d, 16.0)}
    host, dev = {"zeros": z, "wide_range": r}, {"zeros": z_d, "wide_range": r_d}
    for k in range(3):
        s = O.pick_source(c.rowptr, c.seed, k)
        for cls in ("zeros", "wide_range", "zeros"):
            ref, _ = O.sssp_bellman_ford(c.rowptr, c.adj, host[cls], s)
            refw, _ = O.sswp_bellman_ford(c.rowptr, c.adj, host[cls], s)
            for mode in (api.SSSP_PULL, api.SSSP_DIRECTION_OPT):
                d, _ = api.sssp(c.g, dev[cls], s, mode, plan=pull[cls])
                same(d, ref, "pull plan of %s, source %d, mode %d" % (cls, s, mode))
                wd, _ = api.sswp(c.g, dev[cls], s, mode, plan=pull[cls])
                same(wd, refw, "pull plan of %s (widest), source %d, mode %d" % (cls, s, mode))
            d, _ = api.sssp(c.g, None, s, plan=bucketed[cls])
            same(d, ref, "delta plan of %s, source %d" % (cls, s))
    for p in list(pull.values()) + list(bucketed.values()):
        p.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# e. determinism under mass ties
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", MAIN)
def test_two_runs_of_every_schedule_agree_under_ties(gname, ctx, oracle, monkeypatch):
    from vectorgraphlibrary_amd import api
    c = case(ctx, oracle, gname)
    w_d, w, ref = values(ctx, oracle, c, "sssp", "small_ints")
    first, second = run_all_sssp(api, monkeypatch, c, w_d, w, "small_ints"), run_all_sssp(api, monkeypatch, c, w_d, w, "small_ints")
    for (label, a), (_, b) in zip(first, second):
        assert (bits(a) == bits(b)).all(), "SSSP %s: two runs differ" % label
        same(a, ref, label)
    cap_d, cap, refw = values(ctx, oracle, c, "sswp", "ones")
    first, second = run_all_sswp(api, monkeypatch, c, cap_d), run_all_sswp(api, monkeypatch, c, cap_d)
    for (label, a), (_, b) in zip(first, second):
        assert (bits(a) == bits(b)).all(), "SSWP %s: two runs differ" % label
        same(a, refw, label)
