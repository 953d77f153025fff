"""GPU parity tests (run with -m gpu on a MI355X): the HIP path through the C ABI against the CPU oracle on the same
seeded inputs and against the committed golden vectors of the genuine reference.  Integer / f32-distance results are
required to be bit-exact; PageRank within 1e-6 relative of the oracle (tolerance from BASELINE.json north_star)."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = sorted(p for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")) if not os.path.basename(p).startswith(("hits_", "scc_")))
HITS_GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "hits_*.npz")))
SCC_GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "scc_*.npz")))
PR_RTOL = 1e-6


def relerr(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b) / np.maximum(np.abs(b.astype(np.float64)), 1e-300)))


def build_case(ctx, O, kind, scale, ef, seed, symmetric=False):
    from vectorgraphlibrary_amd import api
    V = 1 << scale
    gen_d = ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform
    gen_h = O.gen_rmat if kind == "rmat" else O.gen_uniform
    src, dst = gen_d(scale, ef, seed)
    hs, hd = gen_h(scale, ef, seed)
    assert (src.cpu().numpy() == hs).all() and (dst.cpu().numpy() == hd).all(), "device generator != oracle generator"
    if symmetric:
        import torch
        src, dst = torch.cat([src, dst]), torch.cat([dst, src])
        hs, hd = O.symmetrize(hs, hd)
    g = api.Graph.from_coo(ctx, V, src, dst, want_perm=True)
    rowptr, adj, perm = O.coo_to_csr(V, hs, hd)
    assert (g.out_rowptr.cpu().numpy() == rowptr).all(), "device CSR offsets != oracle"
    assert (g.out_adj.cpu().numpy() == adj).all(), "device CSR adjacency != oracle (stable order)"
    assert (g.perm.cpu().numpy() == perm).all()
    return g, V, hs, hd, rowptr, adj, perm


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_algorithms_match_oracle_and_golden(path, ctx, oracle):
    from vectorgraphlibrary_amd import api
    O = oracle
    z = np.load(path)
    kind, scale, ef, seed = str(z["kind"]), int(z["scale"]), int(z["edge_factor"]), int(z["seed"])
    g, V, hs, hd, rowptr, adj, perm = build_case(ctx, O, kind, scale, ef, seed)
    source = int(z["source"])
    full = "levels" in z.files

    # weights: device generator == oracle generator, CSR order through the permutation
    w_in_d = ctx.gen_weights(len(hs), seed)
    w_in = O.gen_weights(len(hs), seed)
    assert (w_in_d.cpu().numpy().view(np.int32) == w_in.view(np.int32)).all()
    w_d = ctx.gather_u32(g.perm, w_in_d)
    w = w_in[perm]

    # ---- BFS: top-down (reference algorithm) and direction-optimising ----
    ref_levels, ref_st = O.bfs_top_down(rowptr, adj, source)
    for mode in (api.BFS_TOP_DOWN, api.BFS_DIRECTION_OPT):
        levels, st = api.bfs(g, source, mode)
        lv = levels.cpu().numpy()
        assert (lv == ref_levels).all(), f"BFS mode {mode}: levels differ from the oracle"
        assert O.fnv1a64(lv) == int(z["bfs_fnv"]), "BFS levels differ from the reference golden"
        assert st["discovered"] == ref_st["discovered"] and st["frontier_total"] == ref_st["frontier_total"]
        if mode == api.BFS_TOP_DOWN:
            assert st["edges_examined"] == ref_st["edges_examined"] and st["levels"] == ref_st["levels"]
    if full:
        assert (lv == z["levels"]).all()

    # ---- SSSP: both schedules reach the same bit-exact fixed point ----
    ref_dist, _ = O.sssp_bellman_ford(rowptr, adj, w, source)
    for mode in (api.SSSP_ALL_ACTIVE, api.SSSP_ACTIVE_TILES, api.SSSP_DELTA_STEPPING, api.SSSP_PULL, api.SSSP_DIRECTION_OPT):
        dist, st = api.sssp(g, w_d, source, mode)
        dv = dist.cpu().numpy()
        assert (dv.view(np.int32) == ref_dist.view(np.int32)).all(), f"SSSP mode {mode}: distances differ from the oracle"
        assert O.fnv1a64(dv) == int(z["sssp_fnv"])
        if mode == api.SSSP_PULL:
            assert st["pull_steps"] == st["iterations"] and st["push_steps"] == 0
    if full:
        assert (dv.view(np.int32) == z["dist"].view(np.int32)).all()

    # ---- SSWP (f1 widening): widest paths on the same capacities, both schedules, bit-exact (only min / max of the inputs) ----
    ref_width, _ = O.sswp_bellman_ford(rowptr, adj, w, source)
    for mode in (api.SSSP_ALL_ACTIVE, api.SSSP_ACTIVE_TILES, api.SSSP_PULL, api.SSSP_DIRECTION_OPT):
        width, st = api.sswp(g, w_d, source, mode)
        wv = width.cpu().numpy()
        assert (wv.view(np.int32) == ref_width.view(np.int32)).all(), f"SSWP mode {mode}: widths differ from the oracle"
        assert O.fnv1a64(wv) == int(z["sswp_fnv"]), "SSWP widths differ from the reference golden"
    assert wv[source] == np.float32(3.4028234663852886e38) and (wv[ref_levels < 0] == 0).all()      # FLT_MAX at the source, 0 where unreachable
    if full:
        assert (wv.view(np.int32) == z["width"].view(np.int32)).all()
    else:
        assert (wv[z["sample_idx"]].view(np.int32) == z["width_s"].view(np.int32)).all()

    # ---- PageRank ----
    it = int(z["pr_iters"])
    ranks, st = api.page_rank(g, it)
    rk = ranks.cpu().numpy()
    ref_rk = O.pagerank(rowptr, adj, it, 1)
    assert relerr(rk, ref_rk) <= PR_RTOL
    assert (rk.view(np.int32) == ref_rk.view(np.int32)).all(), "PageRank not bit-identical to the oracle's f32 evaluation order"
    assert abs(st["ranks_sum"] - float(ref_rk.astype(np.float64).sum())) < 1e-9
    tol = max(PR_RTOL, float(z["pr_ref_csr_vs_vcsr"]))
    if full:
        assert relerr(rk, z["pr_vgl_csr"]) <= tol
    else:
        assert relerr(rk[z["sample_idx"]], z["pr_vgl_csr_s"]) <= tol
    # caller-supplied in-degrees give the same result
    import torch
    indeg = torch.from_numpy(O.indegree_noloops(rowptr, adj)).to(ctx.device)
    ranks2, _ = api.page_rank(g, it, indeg_noloops=indeg)
    assert (ranks2.cpu().numpy().view(np.int32) == rk.view(np.int32)).all()
    g.close()

    # ---- CC on the symmetrised graph ----
    gs, V, hs2, hd2, rp2, adj2, _ = build_case(ctx, O, kind, scale, ef, seed, symmetric=True)
    comp, st = api.connected_components(gs)
    cv = comp.cpu().numpy()
    ref_comp, _ = O.cc_sv(rp2, adj2)
    assert (cv == ref_comp).all(), "CC labels differ from the oracle"
    assert O.fnv1a64(cv) == int(z["cc_fnv"])
    if full:
        assert (cv == z["comp_csr"]).all()
    gs.close()


def test_directed_cc_and_unreachable(ctx, oracle):
    """labels on a DIRECTED graph are min{u : u reaches v}; BFS/SSSP leave unreachable vertices at -1 / FLT_MAX."""
    from vectorgraphlibrary_amd import api
    O = oracle
    g, V, hs, hd, rowptr, adj, perm = build_case(ctx, O, "rmat", 11, 2, 77)
    comp, _ = api.connected_components(g)
    assert (comp.cpu().numpy() == O.cc_sv(rowptr, adj)[0]).all()
    source = O.pick_source(rowptr, 77)
    levels, st = api.bfs(g, source, api.BFS_DIRECTION_OPT)
    ref, _ = O.bfs_top_down(rowptr, adj, source)
    assert (levels.cpu().numpy() == ref).all() and (ref == -1).sum() > 0
    w = O.gen_weights(len(hs), 77)[perm]
    import torch
    dist, _ = api.sssp(g, torch.from_numpy(w).to(ctx.device), source)
    dref, _ = O.sssp_bellman_ford(rowptr, adj, w, source)
    assert (dist.cpu().numpy().view(np.int32) == dref.view(np.int32)).all()
    assert (dref == np.float32(3.4028234663852886e38)).sum() > 0
    g.close()


def test_tiny_and_ragged_graphs(ctx, oracle):
    """hand-made inputs: isolated vertices, self loops, duplicates, V not a multiple of the tile / wave sizes, a hub row
    spanning several edge tiles, empty rows at both ends."""
    import torch
    from vectorgraphlibrary_amd import api
    O = oracle
    rng = np.random.default_rng(5)
    V = 1000
    hub = np.full(5000, 7, np.int32)                     # row 7 spans > 2 tiles
    src = np.concatenate([hub, rng.integers(10, 900, 3000).astype(np.int32), np.array([7, 7, 950], np.int32)])
    dst = np.concatenate([rng.integers(0, V, 5000).astype(np.int32), rng.integers(0, 990, 3000).astype(np.int32),
                          np.array([7, 7, 950], np.int32)])
    s_d, d_d = torch.from_numpy(src).to(ctx.device), torch.from_numpy(dst).to(ctx.device)
    g = api.Graph.from_coo(ctx, V, s_d, d_d, want_perm=True)
    rowptr, adj, perm = O.coo_to_csr(V, src, dst)
    assert (g.out_adj.cpu().numpy() == adj).all() and (g.out_rowptr.cpu().numpy() == rowptr).all()
    for source in (7, 10 + int(np.argmax(np.diff(rowptr)[10:900] > 0))):
        ref, _ = O.bfs_top_down(rowptr, adj, source)
        for mode in (api.BFS_TOP_DOWN, api.BFS_DIRECTION_OPT):
            assert (api.bfs(g, source, mode)[0].cpu().numpy() == ref).all()
    w = O.gen_weights(len(src), 1)[perm]
    dref, _ = O.sssp_bellman_ford(rowptr, adj, w, 7)
    for mode in (api.SSSP_ALL_ACTIVE, api.SSSP_ACTIVE_TILES, api.SSSP_DELTA_STEPPING):
        d, _ = api.sssp(g, torch.from_numpy(w).to(ctx.device), 7, mode)
        assert (d.cpu().numpy().view(np.int32) == dref.view(np.int32)).all()
    assert (api.connected_components(g)[0].cpu().numpy() == O.cc_sv(rowptr, adj)[0]).all()
    rk, _ = api.page_rank(g, 4)
    ref_rk = O.pagerank(rowptr, adj, 4, 1)
    assert (rk.cpu().numpy().view(np.int32) == ref_rk.view(np.int32)).all()
    # zero PageRank iterations = the initial vector (pr.hpp:39-44)
    assert (api.page_rank(g, 0)[0].cpu().numpy() == np.float32(1.0 / V)).all()
    g.close()


def test_frontier_gnf_reduce(ctx, oracle):
    """generic frontier API: set_all_active / clear / add_vertex / generate_new_frontier / reduce
    (base_frontier.h, multicore/generate_new_frontier.hpp:113-164, multicore/reduce.hpp)."""
    import torch
    from vectorgraphlibrary_amd import api, lib
    O = oracle
    g, V, hs, hd, rowptr, adj, perm = build_case(ctx, O, "rmat", 13, 8, 9)
    deg = np.diff(rowptr)
    f = api.Frontier(g)
    assert f.info() == (V, len(adj), api.ALL_ACTIVE)
    vals = torch.arange(V, dtype=torch.int32, device=ctx.device)
    assert f.reduce_sum(vals) == V * (V - 1) // 2
    f.clear()
    assert f.size() == 0
    f.add_vertex(5)
    assert f.info() == (1, int(deg[5]), api.SPARSE) and f.ids().tolist() == [5]
    with pytest.raises(lib.VglHipError):
        f.add_vertex(6)                                   # only into an empty frontier (modification.hpp:33-36)
    rng = np.random.default_rng(3)
    for p in (0.0, 0.001, 0.3, 0.9, 1.0):
        flags = (rng.random(V) < p).astype(np.int32) * 3  # any non-zero value counts
        if p == 1.0:
            flags[:] = 1
        fl = torch.from_numpy(flags).to(ctx.device)
        f.generate_from_flags(fl)
        size, neigh, kind = f.info()
        want = np.flatnonzero(flags).astype(np.int32)
        assert size == len(want) and neigh == int(deg[want].sum())
        assert kind == (api.ALL_ACTIVE if size == V else api.SPARSE)
        if kind == api.SPARSE:
            assert (f.ids().numpy() == want).all()        # ascending ids
        assert (f.flags().numpy() == (flags != 0)).all()
        fv = torch.from_numpy(rng.random(V).astype(np.float32)).to(ctx.device)
        assert abs(f.reduce_sum(fv) - float(fv.cpu().numpy().astype(np.float64)[want].sum())) < 1e-6
        assert f.reduce_sum(vals) == int(want.astype(np.int64).sum())
        f.generate_from_flags(fl, dense_threshold=0.7)    # VectCSR rule (generate_new_frontier.hpp:67-91)
        if V > size > 0.7 * V:
            assert f.info()[2] == api.DENSE
            assert f.reduce_sum(vals) == int(want.astype(np.int64).sum())
    levels = torch.from_numpy(rng.integers(-1, 4, V).astype(np.int32)).to(ctx.device)
    f.generate_equal(levels, 2)
    assert (f.ids().numpy() == np.flatnonzero(levels.cpu().numpy() == 2)).all()
    a = torch.from_numpy(rng.integers(0, 3, V).astype(np.int32)).to(ctx.device)
    b = torch.from_numpy(rng.integers(0, 3, V).astype(np.int32)).to(ctx.device)
    assert api.count_not_equal(ctx, a, b) == int((a != b).sum())
    f.close()
    g.close()


def test_sharded_super_steps_single_process(ctx, oracle):
    """edge-cut shards driven from one process: the per-shard kernels + the bitmap / min exchange reproduce the
    single-GPU results (the multi-process version of the same protocol is covered with gloo in test_distributed_cpu)."""
    import torch
    from vectorgraphlibrary_amd import api
    from protocol_model import HipShardOps
    O = oracle
    g, V, hs, hd, rowptr, adj, perm = build_case(ctx, O, "rmat", 12, 16, 21)
    w = ctx.gather_u32(g.perm, ctx.gen_weights(len(hs), 21))
    source = O.pick_source(rowptr, 21)
    P = 3
    bounds = ctx.partition_rows(g.out_rowptr, P)
    assert bounds[0] == 0 and bounds[-1] == V and all(b % 64 == 0 for b in bounds[:-1]) and bounds == sorted(bounds)
    edges = [int(rowptr[bounds[p + 1]] - rowptr[bounds[p]]) for p in range(P)]
    assert max(edges) < 1.5 * len(adj) / P + 64 * int(np.diff(rowptr).max())
    shards, ops = [], []
    for p in range(P):
        s = g.shard(bounds[p], bounds[p + 1])
        lo, hi = g.out_edge_range(bounds[p], bounds[p + 1])
        shards.append(s)
        ops.append(HipShardOps(s, w[lo:hi].clone()))
    words = (V + 63) // 64

    # BFS: every shard expands its part of the frontier on its own replica, bitmaps are OR-ed
    reps = [o.new_i32() for o in ops]
    for o, r in zip(ops, reps):
        o.bfs_init(r, source)
    level = 1
    while True:
        everyone = ops[0].new_words(P)
        for p, (o, r) in enumerate(zip(ops, reps)):
            o.bfs_step(r, level)
            o.levels_to_bitmap(r, level + 1, everyone[p * words:(p + 1) * words])
        newly = [o.apply_bitmaps(P, everyone, r, level + 1)[0] for o, r in zip(ops, reps)]
        assert len(set(newly)) == 1
        if newly[0] == 0:
            break
        level += 1
    ref, _ = O.bfs_top_down(rowptr, adj, source)
    for r in reps:
        assert (r.cpu().numpy() == ref).all()

    # the driver itself (world size 1, one shard = whole graph): top-down and direction-optimising must agree with the oracle
    import protocol_model as vd
    whole = HipShardOps(g, w)
    degrees = (g.out_rowptr[1:] - g.out_rowptr[:-1]).to(torch.int32)
    assert (vd.bfs_sharded(whole, source)[0].cpu().numpy() == ref).all()
    assert (vd.bfs_sharded(whole, source, degrees=degrees, edges=len(adj))[0].cpu().numpy() == ref).all()
    # bottom-up step on shards: every shard scans its own rows, bitmaps are OR-ed
    reps = [o.new_i32() for o in ops]
    for o, r in zip(ops, reps):
        o.bfs_init(r, source)
    vis = [o.new_words(1) for o in ops]
    fr = [o.new_words(1) for o in ops]
    for o, r, v_, f_ in zip(ops, reps, vis, fr):
        o.levels_to_bitmap(r, 1, f_)
        v_.copy_(f_)
    level = 1
    while True:
        everyone = ops[0].new_words(P)
        for p, (o, r) in enumerate(zip(ops, reps)):
            o.bfs_step_bu(r, level, vis[p], fr[p], everyone[p * words:(p + 1) * words])
        res = [o.apply_bitmaps(P, everyone, r, level + 1, vis[p], fr[p], degrees) for p, (o, r) in enumerate(zip(ops, reps))]
        assert len(set(res)) == 1
        if res[0][0] == 0:
            break
        level += 1
    for r in reps:
        assert (r.cpu().numpy() == ref).all(), "sharded bottom-up BFS differs from the oracle"

    # SSSP: relax owned rows, elementwise min across replicas
    reps = [o.new_f32() for o in ops]
    for o, r in zip(ops, reps):
        o.sssp_init(r, source)
    while True:
        ch = [o.sssp_relax(r) for o, r in zip(ops, reps)]
        m = torch.stack(reps).min(dim=0).values
        for r in reps:
            r.copy_(m)
        if not any(ch):
            break
    dref, _ = O.sssp_bellman_ford(rowptr, adj, O.gen_weights(len(hs), 21)[perm], source)
    assert (reps[0].cpu().numpy().view(np.int32) == dref.view(np.int32)).all()

    # SSWP: relax owned rows, elementwise max across replicas
    reps = [o.new_f32() for o in ops]
    for o, r in zip(ops, reps):
        o.sswp_init(r, source)
    while True:
        ch = [o.sswp_relax(r) for o, r in zip(ops, reps)]
        m = torch.stack(reps).max(dim=0).values
        for r in reps:
            r.copy_(m)
        if not any(ch):
            break
    wref, _ = O.sswp_bellman_ford(rowptr, adj, O.gen_weights(len(hs), 21)[perm], source)
    assert (reps[0].cpu().numpy().view(np.int32) == wref.view(np.int32)).all()

    # CC (directed labels) and PageRank with owned-slice exchange
    reps = [o.new_i32() for o in ops]
    for o, r in zip(ops, reps):
        o.cc_init(r)
    while True:
        ch = [o.cc_hook(r) for o, r in zip(ops, reps)]
        m = torch.stack(reps).min(dim=0).values
        for r in reps:
            r.copy_(m)
        if not any(ch):
            break
        for o, r in zip(ops, reps):
            o.cc_jump(r)
    assert (reps[0].cpu().numpy() == O.cc_sv(rowptr, adj)[0]).all()

    indeg = ops[0].new_i32()
    indeg.zero_()
    for o in ops:
        o.indeg_add(indeg)
    assert (indeg.cpu().numpy() == O.indegree_noloops(rowptr, adj)).all()
    ranks, rdeg, contrib = ops[0].new_f32(), ops[0].new_f32(), ops[0].new_f32()
    ops[0].pr_setup(indeg, ranks, rdeg)
    for _ in range(5):
        new = [ranks.clone() for _ in range(P)]
        for p, o in enumerate(ops):
            o.pr_iteration(indeg, rdeg, new[p], contrib)
        for p in range(P):
            ranks[bounds[p]:bounds[p + 1]] = new[p][bounds[p]:bounds[p + 1]]
    assert (ranks.cpu().numpy().view(np.int32) == O.pagerank(rowptr, adj, 5, 1).view(np.int32)).all()
    for s in shards:
        s.close()
    g.close()


@pytest.mark.parametrize("kind,scale", [("rmat", 20), ("ru", 20)])
def test_large_scale_properties(kind, scale, ctx):
    """size-independent invariants at a scale the CPU oracle is not asked to run in the GPU suite:
    DO-BFS == top-down BFS, BFS level consistency over every edge, SSSP fixed point (no violated edge, every
    finite distance is tight through some in-edge), CC labels closed under edges and idempotent, PageRank mass."""
    import torch
    from vectorgraphlibrary_amd import api
    ef, seed = 16, 11
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    g = api.Graph.from_coo(ctx, V, src, dst, want_perm=True)
    deg = g.out_rowptr[1:] - g.out_rowptr[:-1]
    source = int(torch.argmax((deg > 0).to(torch.int32)))
    csr_src = torch.repeat_interleave(torch.arange(V, device=ctx.device), deg)
    adj = g.out_adj.long()

    lv_td, st_td = api.bfs(g, source, api.BFS_TOP_DOWN)
    lv_do, st_do = api.bfs(g, source, api.BFS_DIRECTION_OPT)
    assert torch.equal(lv_td, lv_do)
    assert st_do["edges_examined"] <= st_td["edges_examined"]
    ls, ld = lv_td[csr_src], lv_td[adj]
    reached = ls > 0
    assert bool((ld[reached] > 0).all()) and bool((ld[reached] <= ls[reached] + 1).all())
    assert int(lv_td[source]) == 1 and int((lv_td == 1).sum()) == 1
    # every reached non-source vertex has a parent one level up
    best = torch.full((V,), 1 << 30, dtype=torch.int32, device=ctx.device)
    best.scatter_reduce_(0, adj[reached], ls[reached], reduce="amin")
    nz = (lv_td > 1)
    assert bool((best[nz] == lv_td[nz] - 1).all())

    w = ctx.gather_u32(g.perm, ctx.gen_weights(src.numel(), seed))
    d1, s1 = api.sssp(g, w, source, api.SSSP_ACTIVE_TILES)
    d2, s2 = api.sssp(g, w, source, api.SSSP_ALL_ACTIVE)
    assert torch.equal(d1.view(torch.int32), d2.view(torch.int32))
    for delta in (3.0, 16.0, 1000.0):
        d3, s3 = api.sssp(g, w, source, api.SSSP_DELTA_STEPPING, delta=delta)
        assert torch.equal(d1.view(torch.int32), d3.view(torch.int32)), f"delta-stepping (delta={delta}) changed the distances"
    # frontier selection of delta-stepping steps: one pass with a packed atomic reservation per workgroup (the default), count + scan +
    # write, and the per-tile single pass for steps predicted small; forcing each must not change a bit (the switches are read per run)
    import os
    for wide, small in (("1", "4096"), ("0", "0"), ("0", "1000000000")):
        os.environ["VGL_DS_WIDE"], os.environ["VGL_DS_SMALL"] = wide, small
        try:
            d4, _ = api.sssp(g, w, source, api.SSSP_DELTA_STEPPING, delta=16.0)
        finally:
            del os.environ["VGL_DS_SMALL"], os.environ["VGL_DS_WIDE"]
        assert torch.equal(d1.view(torch.int32), d4.view(torch.int32)), f"VGL_DS_WIDE={wide} VGL_DS_SMALL={small}"
    # round 4: dense steps as blocked passes over the heavy part (1) or both parts (2), every step forced dense, with and without fused tiles
    for blocked, fuse in (("1", "0"), ("2", "0"), ("2", "64")):
        os.environ["VGL_DS_BLOCKED"], os.environ["VGL_BLK_FUSE_MIN"], os.environ["VGL_DS_DENSE"], os.environ["VGL_DS_DENSE_BLK"] = blocked, fuse, "0", "0"
        try:
            for delta in (3.0, 16.0):
                d5, _ = api.sssp(g, w, source, api.SSSP_DELTA_STEPPING, delta=delta)
                assert torch.equal(d1.view(torch.int32), d5.view(torch.int32)), f"VGL_DS_BLOCKED={blocked} fuse {fuse} delta {delta}"
        finally:
            del os.environ["VGL_DS_BLOCKED"], os.environ["VGL_BLK_FUSE_MIN"], os.environ["VGL_DS_DENSE"], os.environ["VGL_DS_DENSE_BLK"]
    assert s1["edges_relaxed"] <= s2["edges_relaxed"]
    fin = d1[csr_src] < 3.0e38
    cand = d1[csr_src][fin] + w[fin]
    assert bool((d1[adj[fin]] <= cand).all())                       # no violated edge
    tight = torch.full((V,), float("inf"), device=ctx.device)
    tight.scatter_reduce_(0, adj[fin], cand, reduce="amin")
    m = (d1 < 3.0e38)
    m[source] = False
    assert torch.equal(tight[m], d1[m])                             # every finite distance is realised by an in-edge
    assert torch.equal(d1 < 3.0e38, lv_td > 0)                      # same reachable set as BFS

    comp, _ = api.connected_components(g)
    assert bool((comp[comp.long()] == comp).all()) and bool((comp[adj] <= comp[csr_src]).all())
    assert bool((comp <= torch.arange(V, device=ctx.device)).all())

    ranks, st = api.page_rank(g, 3)
    assert bool((ranks > 0).all()) and abs(st["ranks_sum"] - float(ranks.double().sum())) < 1e-9
    g.close()


@pytest.mark.parametrize("kind", ["out", "in", "total"])
@pytest.mark.parametrize("case", ["rmat_s12_e16_seed3", "ru_s12_e16_seed5"])
def test_degree_renumbered_graph(kind, case, ctx, oracle):
    """VectCSR-style renumbering (vect_csr/import.hpp:61-99): order = (degree desc, id asc) as the oracle's
    vgo_degree_renumber; all four algorithms on the renumbered graph give the ORIGINAL-numbering results of the goldens."""
    import torch
    from vectorgraphlibrary_amd import api
    O = oracle
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", case + ".npz"))
    gk, scale, ef, seed = str(z["kind"]), int(z["scale"]), int(z["edge_factor"]), int(z["seed"])
    V = 1 << scale
    src, dst = (ctx.gen_rmat if gk == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    hs, hd = (O.gen_rmat if gk == "rmat" else O.gen_uniform)(scale, ef, seed)
    g = api.Graph.from_coo(ctx, V, src, dst, want_perm=True, renumber=kind)
    # the order itself, against the oracle's restatement of the reference rule
    deg_src = {"out": hs, "in": hd, "total": np.concatenate([hs, hd])}[kind]
    fake_rowptr = np.concatenate([[0], np.cumsum(np.bincount(deg_src, minlength=V))]).astype(np.int64)
    fwd, bwd = O.degree_renumber(fake_rowptr)
    assert (g.fwd.cpu().numpy() == fwd).all() and (g.bwd.cpu().numpy() == bwd).all()
    rowptr, adj, perm = O.coo_to_csr(V, fwd[hs], fwd[hd])
    assert (g.out_adj.cpu().numpy() == adj).all() and (g.out_rowptr.cpu().numpy() == rowptr).all()
    source = int(z["source"])
    for mode in (api.BFS_TOP_DOWN, api.BFS_DIRECTION_OPT):
        assert (api.bfs(g, source, mode)[0].cpu().numpy() == z["levels"]).all()
    w = ctx.gather_u32(g.perm, ctx.gen_weights(len(hs), seed))
    for mode in (api.SSSP_ALL_ACTIVE, api.SSSP_ACTIVE_TILES, api.SSSP_DELTA_STEPPING):
        assert (api.sssp(g, w, source, mode)[0].cpu().numpy().view(np.int32) == z["dist"].view(np.int32)).all()
    assert (api.sswp(g, w, source)[0].cpu().numpy().view(np.int32) == z["width"].view(np.int32)).all()
    rk = api.page_rank(g, int(z["pr_iters"]))[0].cpu().numpy()
    ref = O.pagerank(*O.coo_to_csr(V, hs, hd)[:2], int(z["pr_iters"]), 1)
    assert relerr(rk, ref) <= PR_RTOL
    g.close()
    s2, d2 = torch.cat([src, dst]), torch.cat([dst, src])
    gs = api.Graph.from_coo(ctx, V, s2, d2, renumber=kind)
    assert (api.connected_components(gs)[0].cpu().numpy() == z["comp_csr"]).all()
    gs.close()


@pytest.mark.parametrize("V,edges", [(1, []), (1, [(0, 0)]), (5, []), (5, [(0, 1), (1, 2), (4, 4), (2, 0)]), (70, [(69, 0), (0, 69), (3, 3)])])
def test_degenerate_graphs(V, edges, ctx, oracle):
    """smallest inputs: a single vertex, no edges at all, only a self loop, V below one wavefront / one bitmap word."""
    import torch
    from vectorgraphlibrary_amd import api
    O = oracle
    src = np.array([e[0] for e in edges], np.int32)
    dst = np.array([e[1] for e in edges], np.int32)
    g = api.Graph.from_coo(ctx, V, torch.from_numpy(src).to(ctx.device), torch.from_numpy(dst).to(ctx.device), want_perm=True)
    rowptr, adj, perm = O.coo_to_csr(V, src, dst)
    assert (g.out_rowptr.cpu().numpy() == rowptr).all()
    for source in {0, V - 1}:
        ref, _ = O.bfs_top_down(rowptr, adj, source)
        for mode in (api.BFS_TOP_DOWN, api.BFS_DIRECTION_OPT):
            lv, st = api.bfs(g, source, mode)
            assert (lv.cpu().numpy() == ref).all() and st["discovered"] == int((ref > 0).sum())
        w = np.linspace(1.0, 2.0, len(src), dtype=np.float32)[perm] if len(src) else np.zeros(0, np.float32)
        w_d = torch.from_numpy(w).to(ctx.device) if len(src) else torch.zeros(1, device=ctx.device)
        dref, _ = O.sssp_bellman_ford(rowptr, adj, w, source)
        for mode in (api.SSSP_ALL_ACTIVE, api.SSSP_ACTIVE_TILES, api.SSSP_DELTA_STEPPING):
            d, _ = api.sssp(g, w_d, source, mode, delta=0.5)
            assert (d.cpu().numpy().view(np.int32) == dref.view(np.int32)).all()
        wref, _ = O.sswp_bellman_ford(rowptr, adj, w, source)
        for mode in (api.SSSP_ALL_ACTIVE, api.SSSP_ACTIVE_TILES):
            assert (api.sswp(g, w_d, source, mode)[0].cpu().numpy().view(np.int32) == wref.view(np.int32)).all()
    assert (api.connected_components(g)[0].cpu().numpy() == O.cc_sv(rowptr, adj)[0]).all()
    rk = api.page_rank(g, 3)[0].cpu().numpy()
    assert (rk.view(np.int32) == O.pagerank(rowptr, adj, 3, 1).view(np.int32)).all()
    f = api.Frontier(g)
    assert f.info() == (V, len(src), api.ALL_ACTIVE)
    f.generate_from_flags(torch.zeros(V, dtype=torch.int32, device=ctx.device))
    assert f.size() == 0 and f.ids().numel() == 0
    f.close()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,renumber,placement", [("rmat", "total", "ranges"), ("rmat", None, "ranges"), ("ru", "out", "ranges"),
                                                     ("rmat", "total", "dealt"), ("ru", None, "dealt")])
def test_generated_shards_match_whole_graph_build(kind, renumber, placement, ctx, oracle):
    """distributed.build_generated_shard (chunked streaming build for graphs larger than one GPU) produces exactly the
    shards Graph.from_coo(...).shard() cuts from the whole graph (incoming lists as per-row multisets), and the sharded
    direction-optimising BFS over them reproduces the oracle's levels."""
    import torch
    from vectorgraphlibrary_amd import api
    import protocol_model as vd
    O = oracle
    scale, ef, seed = 13, 16, 77
    P = 4 if placement == "dealt" else 3
    V, E = 1 << scale, (1 << scale) * ef
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    if placement == "dealt":
        # reference build: relabel the edge list with the shard's own original->stored map, cut equal ranges
        s0, _, bounds = vd.build_generated_shard(ctx, scale, ef, seed, 0, P, kind=kind, renumber=renumber, placement=placement)
        assert bounds == [p * (V // P) for p in range(P + 1)]
        f = s0.fwd
        assert torch.equal(torch.sort(f).values, torch.arange(V, device=ctx.device, dtype=torch.int32))
        assert torch.equal(s0.bwd[f.long()], torch.arange(V, device=ctx.device, dtype=torch.int32))
        if renumber:       # the stored order deals the 64-blocks of the degree order round-robin
            pure = api.Graph.from_coo(ctx, V, src, dst, renumber=renumber, with_incoming=False)
            pos = pure.fwd.long()
            want = ((pos >> 6) % P) * (V // P) + ((pos >> 6) // P) * 64 + (pos & 63)
            assert torch.equal(f.long(), want)
            pure.close()
        whole = api.Graph.from_coo(ctx, V, ctx.relabel(f, src), ctx.relabel(f, dst))
        whole.fwd, whole.bwd = s0.fwd, s0.bwd
        s0.close()
        edges = [int(whole.out_rowptr[bounds[p + 1]] - whole.out_rowptr[bounds[p]]) for p in range(P)]
        assert sum(edges) == E and (kind == "rmat" or max(edges) < 1.25 * E / P), edges   # tiny RMAT: the first 64 hubs dominate
    else:
        whole = api.Graph.from_coo(ctx, V, src, dst, renumber=renumber)
        bounds = ctx.partition_rows(whole.out_rowptr, P)
    shards = []
    for p in range(P):
        s, degrees, b = vd.build_generated_shard(ctx, scale, ef, seed, p, P, kind=kind, renumber=renumber, chunk_edges=30011,
                                                 placement=placement)
        assert b == bounds
        ref = whole.shard(bounds[p], bounds[p + 1])
        assert torch.equal(s.out_rowptr, ref.out_rowptr) and torch.equal(s.out_adj, ref.out_adj)
        assert torch.equal(s.in_rowptr, ref.in_rowptr)
        rows = torch.repeat_interleave(torch.arange(s.in_rowptr.numel() - 1, device=ctx.device), s.in_rowptr[1:] - s.in_rowptr[:-1])
        key = lambda g: torch.sort(rows * V + g.in_adj.to(torch.int64)).values
        assert torch.equal(key(s), key(ref))
        assert torch.equal(degrees, (whole.out_rowptr[1:] - whole.out_rowptr[:-1]).to(torch.int32))
        if renumber or placement == "dealt":
            assert torch.equal(s.fwd, whole.fwd) and torch.equal(s.bwd, whole.bwd)
        # the same shard built in row-range pieces (what a shard with more than 2^31 edges goes through) is the same CSR, incoming
        # adjacency included (pieces keep the generation order inside every row)
        sp, _, _ = vd.build_generated_shard(ctx, scale, ef, seed, p, P, kind=kind, renumber=renumber, chunk_edges=30011, placement=placement,
                                            piece_edges=max(1000, int(s.out_adj.numel()) // 5))
        assert torch.equal(sp.out_rowptr, s.out_rowptr) and torch.equal(sp.out_adj, s.out_adj)
        assert torch.equal(sp.in_rowptr, s.in_rowptr) and torch.equal(sp.in_adj, s.in_adj)
        sp.close()
        ref.close()
        shards.append(s)
    rowptr, adj = whole.out_rowptr.cpu().numpy(), whole.out_adj.cpu().numpy()
    source = O.pick_source(rowptr, seed)
    want, _ = O.bfs_top_down(rowptr, adj, source)
    # shards driven in lock-step from one process (the collective is the concatenation of the per-shard bitmaps)
    ops = [vd.HipShardOps(s) for s in shards]
    words = (V + 63) // 64
    reps = [o.new_i32() for o in ops]
    vis, fr = [o.new_words(1) for o in ops], [o.new_words(1) for o in ops]
    for o, r, v_, f_ in zip(ops, reps, vis, fr):
        o.bfs_init(r, source)
        o.levels_to_bitmap(r, 1, f_)
        v_.copy_(f_)
    level = 1
    while True:
        everyone = ops[0].new_words(P)
        parts, bits = P, everyone
        for p, (o, r) in enumerate(zip(ops, reps)):
            mine = everyone[p * words:(p + 1) * words]
            if level % 3 == 1:
                o.bfs_step_bits(r, level, vis[p], fr[p], mine)
            elif level % 3 == 2:
                o.bfs_step(r, level, vis[p])
                o.levels_to_bitmap(r, level + 1, mine)
            else:
                o.bfs_step_bu(r, level, vis[p], fr[p], mine)
        if placement == "dealt" and level % 3 == 0:          # bottom-up level: owned slices concatenate to the merged bitmap
            lo = [b // 64 for b in bounds]
            parts, bits = 1, torch.cat([everyone[p * words + lo[p]:p * words + lo[p + 1]] for p in range(P)])
        res = [o.apply_bitmaps(parts, bits, r, level + 1, vis[p], fr[p], degrees) for p, (o, r) in enumerate(zip(ops, reps))]
        assert len(set(res)) == 1
        if res[0][0] == 0:
            break
        level += 1
    for r in reps:
        assert (r.cpu().numpy() == want).all()
    # world size 1 through the driver
    one, degrees, _ = vd.build_generated_shard(ctx, scale, ef, seed, 0, 1, kind=kind, renumber=renumber, chunk_edges=50000,
                                               placement=placement)
    got, _ = vd.bfs_sharded(vd.HipShardOps(one), source, degrees=degrees, edges=E)
    if placement == "dealt":       # world 1: dealing is the identity on positions, i.e. the plain renumbered graph
        src1 = one.vertex_id(int(whole.bwd[source]))
        got, _ = vd.bfs_sharded(vd.HipShardOps(one), src1, degrees=degrees, edges=E)
        got = one.to_original(got)
        want1 = whole.to_original(torch.from_numpy(want).to(ctx.device))
        assert torch.equal(got, want1)
    else:
        assert (got.cpu().numpy() == want).all()
    for s in shards + [one]:
        s.close()
    whole.close()


@pytest.mark.gpu
def test_pagerank_indegree_paths_and_hub_schedule(ctx, oracle):
    """PageRank takes the in-degrees from the incoming CSR when the graph has one and from per-edge atomics otherwise; rows with
    >= 512 edges go through the hub schedule.  All of it must reproduce the oracle's sequential f32 sums bit for bit."""
    from vectorgraphlibrary_amd import api
    O = oracle
    scale, ef, seed = 14, 32, 9                      # RMAT-14x32: a few hundred rows above the hub threshold
    V = 1 << scale
    src, dst = ctx.gen_rmat(scale, ef, seed)
    both = api.Graph.from_coo(ctx, V, src, dst, with_incoming=True)
    out_only = api.Graph.from_coo(ctx, V, src, dst, with_incoming=False)
    rowptr, adj = both.out_rowptr.cpu().numpy(), both.out_adj.cpu().numpy()
    assert int(np.diff(rowptr).max()) >= 4 * 512 and int((np.diff(rowptr) >= 512).sum()) > 64
    want = O.pagerank(rowptr, adj, 4, 1)
    a, _ = api.page_rank(both, 4)
    b, _ = api.page_rank(out_only, 4)
    assert (a.cpu().numpy().view(np.int32) == want.view(np.int32)).all()
    assert (b.cpu().numpy().view(np.int32) == want.view(np.int32)).all()
    both.close(); out_only.close()
    # the longest rows as GIANT hubs (a whole workgroup per row: three wavefronts gather, one adds; vgl_pull.h) -- forced from 1000 entries
    # here (default 32768), odd row lengths included -- and with the scheme off: the same bits, the chain's order is the adjacency order
    import os
    for name, value in (("VGL_PULL_GIANT_DEGREE", "1000"), ("VGL_PULL_GIANT_DEGREE", "513"), ("VGL_PULL_NO_GIANTS", "1")):
        os.environ[name] = value
        try:
            g2 = api.Graph.from_coo(ctx, V, src, dst, with_incoming=True)
            c2, _ = api.page_rank(g2, 4)
        finally:
            os.environ.pop(name)
        assert (c2.cpu().numpy().view(np.int32) == want.view(np.int32)).all(), (name, value)
        g2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,scale,ef,renumber", [("rmat", 14, 8, None), ("rmat", 14, 8, "total"), ("ru", 13, 1, None), ("ru", 12, 1, "out")])
def test_symmetric_cc_matches_shiloach_vishkin(kind, scale, ef, renumber, ctx, oracle):
    """on a symmetrised graph the union-find path returns exactly the hook/jump labels (smallest id of the component): against the
    oracle's SV and sequential-BFS labelling, under identity and degree-sorted numbering, on graphs with one giant component (RMAT)
    and with hundreds of small ones (sparse uniform)."""
    import torch
    from vectorgraphlibrary_amd import api
    O = oracle
    V = 1 << scale
    s, d = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, 31)
    src, dst = torch.cat([s, d]), torch.cat([d, s])
    g = api.Graph.from_coo(ctx, V, src, dst, with_incoming=False, renumber=renumber)
    plain = api.Graph.from_coo(ctx, V, src, dst, with_incoming=False) if renumber else g
    rowptr, adj = plain.out_rowptr.cpu().numpy(), plain.out_adj.cpu().numpy()
    want = O.cc_sv(rowptr, adj)[0]
    seq = O.cc_seq_bfs(rowptr, adj)                    # the reference checker's labelling (component counter): same partition,
    mins = np.full(int(seq.max()) + 1, V, np.int64)    # and the SV label is the smallest id of each part
    np.minimum.at(mins, seq, np.arange(V))
    assert (mins[seq] == want).all()
    fast, st = api.connected_components(g, symmetric=True)
    slow, _ = api.connected_components(g)
    assert (fast.cpu().numpy() == want).all()
    assert (slow.cpu().numpy() == want).all()
    assert st["hook_passes"] == 3
    ncomp = len(np.unique(want))
    assert ncomp > (100 if kind == "ru" else 1)
    g.close()
    if renumber:
        plain.close()


HITS_RTOL = 1e-12          # f64; per-vertex sums keep the reference's order, only the norm's summation order differs (~1e-16)


def _relerr64(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


@pytest.mark.gpu
@pytest.mark.parametrize("path", HITS_GOLDEN, ids=[os.path.basename(p)[:-4] for p in HITS_GOLDEN])
def test_hits_matches_oracle_and_golden(path, ctx, oracle):
    """HITS (f1 widening) through vgl_hip_hits_run against the oracle and the reference's fixtures, identity and degree-sorted ids"""
    import torch
    from vectorgraphlibrary_amd import api
    O = oracle
    z = np.load(path)
    kind, scale, ef, seed, steps = str(z["kind"]), int(z["scale"]), int(z["edge_factor"]), int(z["seed"]), int(z["steps"])
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    for renumber in (None, "total"):
        g = api.Graph.from_coo(ctx, V, src, dst, renumber=renumber)
        auth, hub = api.hits(g, steps)
        a, h = auth.cpu().numpy(), hub.cpu().numpy()
        assert _relerr64(a, z["auth_seq"]) <= HITS_RTOL and _relerr64(h, z["hub_seq"]) <= HITS_RTOL
        assert _relerr64(a, z["auth_vgl_csr"]) <= HITS_RTOL and _relerr64(h, z["hub_vgl_csr"]) <= HITS_RTOL
        a2, h2 = api.hits(g, steps)                                    # deterministic: fixed-order norms, sequential chains
        assert torch.equal(a2, auth) and torch.equal(h2, hub)
        g.close()


@pytest.mark.gpu
def test_hits_hub_rows_and_zero_steps(ctx, oracle):
    """rows above the hub threshold in BOTH directions (RMAT-14x32), and steps = 0 leaves the initial all-ones vectors"""
    from vectorgraphlibrary_amd import api
    O = oracle
    scale, ef, seed = 14, 32, 9
    V = 1 << scale
    src, dst = ctx.gen_rmat(scale, ef, seed)
    g = api.Graph.from_coo(ctx, V, src, dst)
    rowptr, adj = g.out_rowptr.cpu().numpy(), g.out_adj.cpu().numpy()
    assert int(np.diff(rowptr).max()) >= 2048 and int(np.diff(g.in_rowptr.cpu().numpy()).max()) >= 2048
    wa, wh = O.hits(rowptr, adj, 3)
    a, h = api.hits(g, 3)
    assert _relerr64(a.cpu().numpy(), wa) <= HITS_RTOL and _relerr64(h.cpu().numpy(), wh) <= HITS_RTOL
    a0, h0 = api.hits(g, 0)
    assert float(a0.min()) == 1.0 == float(a0.max()) and float(h0.min()) == 1.0 == float(h0.max())
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", SCC_GOLDEN, ids=[os.path.basename(p)[:-4] for p in SCC_GOLDEN])
def test_scc_matches_oracle_and_golden(path, ctx, oracle):
    """SCC (f1 widening): vgl_hip_scc_run returns exactly the canonical labels of the reference's Tarjan partition, under identity
    and degree-sorted numbering (including the sparse input on which the reference's own forward-backward code is wrong)"""
    from vectorgraphlibrary_amd import api
    O = oracle
    z = np.load(path)
    kind, scale, ef, seed = str(z["kind"]), int(z["scale"]), int(z["edge_factor"]), int(z["seed"])
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    for renumber in (None, "total"):
        g = api.Graph.from_coo(ctx, V, src, dst, renumber=renumber)
        comp, st = api.strongly_connected_components(g)
        assert (comp.cpu().numpy() == z["comp"]).all(), f"SCC labels differ (renumber={renumber}, stats={st})"
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,scale,ef", [("rmat", 16, 16), ("ru", 16, 1), ("ru", 15, 2)])
def test_scc_larger_graphs_match_oracle(kind, scale, ef, ctx, oracle):
    import torch
    from vectorgraphlibrary_amd import api
    O = oracle
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, 41)
    g = api.Graph.from_coo(ctx, V, src, dst)
    want = O.scc_tarjan(g.out_rowptr.cpu().numpy(), g.out_adj.cpu().numpy())
    comp, st = api.strongly_connected_components(g)
    assert (comp.cpu().numpy() == want).all(), st
    g.close()
    # degenerate: no edges at all, and a single vertex with a self loop
    e = torch.zeros(0, dtype=torch.int32, device=ctx.device)
    g0 = api.Graph.from_coo(ctx, 5, e, e)
    assert (api.strongly_connected_components(g0)[0].cpu().numpy() == np.arange(5)).all()
    g0.close()
    one = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    g1 = api.Graph.from_coo(ctx, 1, one, one)
    assert (api.strongly_connected_components(g1)[0].cpu().numpy() == [0]).all()
    g1.close()


@pytest.mark.gpu
def test_bitmap_or_parts(ctx):
    """the merge step of the two-phase top-down exchange (protocol_model.bfs_sharded): out = OR of the received slices"""
    import torch
    from vectorgraphlibrary_amd import api
    import protocol_model as vd
    V = 64 * 1000
    src = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    g = api.Graph.from_coo(ctx, V, src, src)
    ops = vd.HipShardOps(g)
    P, words = 5, 200
    gen = torch.Generator(device="cpu").manual_seed(3)
    parts = torch.randint(-2**62, 2**62, (P * words,), generator=gen, dtype=torch.int64).to(ctx.device)
    out = torch.empty(words, dtype=torch.int64, device=ctx.device)
    ops.or_parts(P, parts, out)
    want = parts.view(P, words)[0].clone()
    for p in range(1, P):
        want |= parts.view(P, words)[p]
    assert torch.equal(out, want)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(10))
def test_random_graphs_all_algorithms(seed, ctx, oracle):
    """differential sweep over small random graphs of awkward shapes (V not a multiple of 64 / 2048, isolated vertices, self loops,
    duplicate edges, a few hub rows spanning several edge tiles, sometimes no edges at all): every fused algorithm against the oracle"""
    import torch
    from vectorgraphlibrary_amd import api
    O = oracle
    rng = np.random.default_rng(1000 + seed)
    V = int(rng.integers(1, 5000))
    E = int(rng.integers(0, 12 * V + 1)) if seed % 5 else 0
    # skewed endpoints: squaring a uniform variate concentrates edges on low ids (hub rows of thousands of edges)
    src = np.minimum((rng.random(E) ** (1 + seed % 3) * V).astype(np.int32), V - 1)
    dst = np.minimum((rng.random(E) ** (1 + (seed // 3) % 3) * V).astype(np.int32), V - 1)
    rowptr, adj, perm = O.coo_to_csr(V, src, dst)
    w_in = (rng.random(E) * 100).astype(np.float32)
    w = w_in[perm] if E else np.zeros(0, np.float32)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device) if len(a) else torch.zeros(0, dtype=dt, device=ctx.device)
    g = api.Graph.from_coo(ctx, V, dev(src, torch.int32), dev(dst, torch.int32), want_perm=True)
    assert (g.out_rowptr.cpu().numpy() == rowptr).all() and (g.out_adj.cpu().numpy()[:E] == adj).all()
    w_d = ctx.gather_u32(g.perm, dev(w_in, torch.float32)) if E else torch.zeros(1, dtype=torch.float32, device=ctx.device)
    source = int(rng.integers(0, V))
    ref_levels, _ = O.bfs_top_down(rowptr, adj, source)
    for mode in (api.BFS_TOP_DOWN, api.BFS_DIRECTION_OPT):
        assert (api.bfs(g, source, mode)[0].cpu().numpy() == ref_levels).all(), f"BFS mode {mode}"
    ref_dist, _ = O.sssp_bellman_ford(rowptr, adj, w, source)
    for mode in (api.SSSP_ALL_ACTIVE, api.SSSP_ACTIVE_TILES, api.SSSP_DELTA_STEPPING):
        d, _ = api.sssp(g, w_d, source, mode, delta=float(rng.choice([0.5, 7.0, 40.0])))
        assert (d.cpu().numpy().view(np.int32) == ref_dist.view(np.int32)).all(), f"SSSP mode {mode}"
    ref_width, _ = O.sswp_bellman_ford(rowptr, adj, w, source)
    assert (api.sswp(g, w_d, source)[0].cpu().numpy().view(np.int32) == ref_width.view(np.int32)).all()
    assert (api.page_rank(g, 3)[0].cpu().numpy().view(np.int32) == O.pagerank(rowptr, adj, 3, 1).view(np.int32)).all()
    assert (api.connected_components(g)[0].cpu().numpy() == O.cc_sv(rowptr, adj)[0]).all()
    assert (api.strongly_connected_components(g)[0].cpu().numpy() == O.scc_tarjan(rowptr, adj)).all()
    if E:
        wa, wh = O.hits(rowptr, adj, 2)
        a, h = api.hits(g, 2)
        ok = np.isfinite(wa).all() and np.isfinite(wh).all()          # all-zero norms (no edge reaches anything) give NaN in the reference too
        if ok:
            assert _relerr64(a.cpu().numpy(), wa) <= HITS_RTOL and _relerr64(h.cpu().numpy(), wh) <= HITS_RTOL
    g.close()
    # symmetrised: union-find CC == Shiloach-Vishkin labels
    if E:
        s2, d2 = np.concatenate([src, dst]), np.concatenate([dst, src])
        gs = api.Graph.from_coo(ctx, V, dev(s2, torch.int32), dev(d2, torch.int32), with_incoming=False)
        rp2, adj2, _ = O.coo_to_csr(V, s2, d2, want_perm=False)
        want = O.cc_sv(rp2, adj2)[0]
        assert (api.connected_components(gs, symmetric=True)[0].cpu().numpy() == want).all()
        assert (api.connected_components(gs)[0].cpu().numpy() == want).all()
        gs.close()


def test_bfs_batch_equals_single_runs(oracle, ctx):
    """vgl_hip_bfs_run_batch (the bench's timed region: the rounds loop behind one call of the C ABI): per-traversal statistics equal those of
    single calls, the levels buffer holds the last source's levels, an out-of-range source fails the call"""
    import torch
    from vectorgraphlibrary_amd import api
    from vectorgraphlibrary_amd.lib import VglHipError
    O = oracle
    src, dst = O.gen_rmat(12, 16, 7)
    rowptr, adj, _ = O.coo_to_csr(1 << 12, src, dst)
    g = api.Graph.from_coo(ctx, 1 << 12, torch.from_numpy(src).to(ctx.device), torch.from_numpy(dst).to(ctx.device), with_incoming=True)
    sources = [int(np.argmax(np.diff(rowptr))), 5, 77, 1234]
    for mode in (api.BFS_DIRECTION_OPT, api.BFS_TOP_DOWN):
        levels, stats = api.bfs_batch(g, sources, mode)
        assert (levels.cpu().numpy() == O.bfs_top_down(rowptr, adj, sources[-1])[0]).all()
        for s, st in zip(sources, stats):
            one = api.bfs(g, s, mode, raw=True)[1]
            assert st["levels"] == one["levels"] and st["discovered"] == one["discovered"] and st["frontier_total"] == one["frontier_total"]
    with pytest.raises(VglHipError):
        api.bfs_batch(g, [0, 1 << 12], api.BFS_TOP_DOWN)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,scale,ef", [("rmat", 15, 8), ("rmat", 18, 16), ("ru", 16, 8), ("ru", 14, 2), ("ru", 13, 1), ("rmat", 10, 4)])
def test_bfs_small_level_kernel_paths(kind, scale, ef, ctx, oracle):
    """the single-workgroup kernel that runs the first and the last levels of a traversal (vgl_k_bfs_small_levels): off, default and
    with a bound that lets it take whole traversals of sparse graphs -- levels, level count and examined edges must not move"""
    import os
    import torch
    from vectorgraphlibrary_amd import api
    O = oracle
    V = 1 << scale
    src, dst = (O.gen_rmat if kind == "rmat" else O.gen_uniform)(scale, ef, 77)
    rowptr, adj, _ = O.coo_to_csr(V, src, dst)
    g = api.Graph.from_coo(ctx, V, torch.from_numpy(src).to(ctx.device), torch.from_numpy(dst).to(ctx.device))
    nz = np.nonzero(np.diff(rowptr))[0]
    for source in (int(nz[0]), int(nz[len(nz) // 2]), int(np.argmax(np.diff(rowptr)))):
        ref = O.bfs_top_down(rowptr, adj, source)[0]
        for mode in (api.BFS_TOP_DOWN, api.BFS_DIRECTION_OPT):
            seen = []
            # (edge bound of the list kernel, frontier bound of the bitmap-driven level at the bottom-up -> top-down switch, edge bound of the
            # top-down levels that emit their discoveries into the bitmap)
            # ... and VGL_BFS_NO_HINT=1: the count launch before a bottom-up phase walks the new frontier instead of taking F and M from the
            # level that produced it
            for cap, bm, emit, nohint in (("0", None, None, None), (None, None, None, None), ("1000000", None, None, None), (None, "0", None, None),
                                          (None, "1000000000", None, None), ("256", "1000000000", None, None), (None, None, "0", None),
                                          (None, None, "1000000000000", None), ("0", "0", "0", None), (None, None, None, "1"),
                                          ("0", None, "1000000000000", "1"), ("1000000", "0", None, "1")):
                for name, val in (("VGL_BFS_SMALL_M", cap), ("VGL_BFS_BM_EXPAND", bm), ("VGL_TD_EMIT_EDGES", emit), ("VGL_BFS_NO_HINT", nohint)):
                    if val is None:
                        os.environ.pop(name, None)
                    else:
                        os.environ[name] = val
                try:
                    lv, st = api.bfs(g, source, mode)
                finally:
                    for name in ("VGL_BFS_SMALL_M", "VGL_BFS_BM_EXPAND", "VGL_TD_EMIT_EDGES", "VGL_BFS_NO_HINT"):
                        os.environ.pop(name, None)
                assert np.array_equal(lv.cpu().numpy(), ref), (source, mode, cap, bm, emit, nohint)
                seen.append((st["levels"], st["edges_examined"], st["frontier_total"], st["discovered"], st["td_steps"], st["bu_steps"]))
            assert all(x == seen[0] for x in seen), (source, mode, seen)


@pytest.mark.gpu
def test_bfs_level_without_edges_leaves_no_stale_direction_hint(ctx, oracle):
    """a top-down level whose frontier has no out-edges launches no expansion, so it must not announce the frontier size / out-degree sum
    an expansion would have left on the device: the count launch would otherwise read another traversal's (found by tests/studies/fuzz_bfs.py:
    right levels, but a bottom-up step that never happened in the statistics)"""
    import os
    import torch
    from vectorgraphlibrary_amd import api
    O = oracle
    scale, ef = 14, 16
    V = 1 << scale
    src, dst = O.gen_rmat(scale, ef, 5)
    src, dst = src.copy(), dst.copy()
    lonely = V - 1                                      # a vertex without out-edges (its in-edges stay)
    keep = src != lonely
    src, dst = src[keep], dst[keep]
    rowptr, adj, _ = O.coo_to_csr(V, src, dst)
    g = api.Graph.from_coo(ctx, V, torch.from_numpy(src).to(ctx.device), torch.from_numpy(dst).to(ctx.device))
    hub = int(np.argmax(np.diff(rowptr)))
    for small_m in (None, "0"):
        os.environ.pop("VGL_BFS_SMALL_M", None)
        lv, st = api.bfs(g, hub, api.BFS_DIRECTION_OPT)              # leaves the F and M of a real top-down -> bottom-up switch on the device
        assert np.array_equal(lv.cpu().numpy(), O.bfs_top_down(rowptr, adj, hub)[0]) and st["bu_steps"] > 0
        if small_m is not None:
            os.environ["VGL_BFS_SMALL_M"] = small_m                  # list kernel off: the lonely source goes through count / expand launches
        try:
            lv, st = api.bfs(g, lonely, api.BFS_DIRECTION_OPT)
        finally:
            os.environ.pop("VGL_BFS_SMALL_M", None)
        assert np.array_equal(lv.cpu().numpy(), O.bfs_top_down(rowptr, adj, lonely)[0])
        assert (st["levels"], st["discovered"], st["bu_steps"], st["edges_examined"]) == (1, 1, 0, 0), (small_m, st)
    g.close()


@pytest.mark.gpu
def test_sparse_exchange_primitives(ctx):
    """vgl_hip_bitmap_to_ids / vgl_hip_bfs_apply_ids (id-list exchange of tiny multi-GPU levels) against numpy: counts beyond the
    cap are reported, lists are a subset of the set bits, duplicates across parts and visited vertices are taken once / not at all"""
    import torch
    import protocol_model as vd

    class G:                                        # the two calls only need V and the context
        pass
    V = 100003
    g = G(); g.ctx = ctx; g.V = V
    ops = vd.HipShardOps(g)
    rng = np.random.default_rng(5)
    words = (V + 63) // 64

    def pack(ids):
        b = np.zeros(words * 64, np.uint8); b[ids] = 1
        return torch.from_numpy(np.packbits(b, bitorder="little").view(np.int64).copy()).to(ctx.device)

    def unpack(t):
        return np.nonzero(np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[:V])[0]
    for n, cap in ((0, 8), (5, 8), (8, 8), (300, 64), (3000, 4096)):
        ids = np.sort(rng.choice(V, n, replace=False))
        out = ops.new_id_lists(1, cap)
        ops.bits_to_ids(pack(ids), cap, out)
        ops.sync()
        o = out.cpu().numpy()
        assert o[0] == n
        got = o[1:1 + min(n, cap)]
        assert len(set(got.tolist())) == len(got) and set(got.tolist()) <= set(ids.tolist())
        if n <= cap:
            assert sorted(got.tolist()) == ids.tolist()
    cap, parts = 64, 3
    lists = np.zeros((parts, 1 + cap), np.int32)
    a, b, c = rng.choice(V, 40, replace=False), rng.choice(V, 64, replace=False), np.zeros(0, np.int64)
    b[:10] = a[:10]                                                 # reported by two ranks
    for p, l in enumerate((a, b, c)):
        lists[p, 0] = len(l); lists[p, 1:1 + len(l)] = l
    already = np.concatenate([a[20:25], rng.choice(V, 1000, replace=False)])
    visited, front = pack(np.unique(already)), pack(rng.choice(V, 50, replace=False))     # stale frontier bits must disappear
    levels = torch.full((V,), -1, dtype=torch.int32, device=ctx.device)
    levels[torch.from_numpy(np.unique(already)).to(ctx.device)] = 3
    degrees = torch.from_numpy(rng.integers(0, 100, V).astype(np.int32)).to(ctx.device)
    newly, newdeg = ops.apply_ids(parts, cap, torch.from_numpy(lists.reshape(-1)).to(ctx.device), levels, 7, visited, front, degrees)
    expect = np.setdiff1d(np.union1d(a, b), already)
    assert newly == len(expect) and newdeg == int(degrees.cpu().numpy()[expect].sum())
    assert np.array_equal(unpack(front), expect) and np.array_equal(unpack(visited), np.union1d(expect, already))
    lv = levels.cpu().numpy()
    assert (lv[expect] == 7).all() and (lv[np.unique(already)] == 3).all() and (lv == -1).sum() == V - len(expect) - len(np.unique(already))


@pytest.mark.gpu
@pytest.mark.parametrize("renumber", [None, "total", "out", "in"])
def test_edgeless_graph_with_renumbering(renumber, ctx):
    """no edges at all (the arrays of an empty edge list are null pointers): build, renumber, traverse"""
    import torch
    from vectorgraphlibrary_amd import api
    V = 1000
    e = torch.zeros(0, dtype=torch.int32, device=ctx.device)
    g = api.Graph.from_coo(ctx, V, e, e, renumber=renumber)
    for mode in (api.BFS_TOP_DOWN, api.BFS_DIRECTION_OPT):
        lv, st = api.bfs(g, 7, mode)
        assert int(lv[7]) == 1 and int((lv == -1).sum()) == V - 1 and st["levels"] == 1
    comp, _ = api.connected_components(g)
    assert torch.equal(comp.cpu(), torch.arange(V, dtype=torch.int32))
    g.close()


@pytest.mark.gpu
def test_apply_bitmaps_owned(ctx):
    """vgl_hip_bfs_apply_bitmaps_owned: bitmaps updated for every vertex, levels / counts / degree sums for the owned range only"""
    import torch
    import protocol_model as vd

    class G:
        pass
    V, lo, hi = 100000, 12800, 51200
    g = G(); g.ctx = ctx; g.V = V; g.row_begin = lo; g.row_end = hi
    ops = vd.HipShardOps(g)
    rng = np.random.default_rng(11)
    words = (V + 63) // 64

    def pack(mask):
        b = np.zeros(words * 64, np.uint8); b[:V] = mask
        return torch.from_numpy(np.packbits(b, bitorder="little").view(np.int64).copy()).to(ctx.device)

    def unpack(t):
        return np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[:V].astype(bool)
    parts = [rng.random(V) < 0.05 for _ in range(3)]
    visited0 = rng.random(V) < 0.3
    bits_all = torch.cat([pack(p) for p in parts])
    visited, front = pack(visited0), pack(rng.random(V) < 0.5)
    levels = torch.full((V,), -1, dtype=torch.int32, device=ctx.device)
    degrees = torch.from_numpy(rng.integers(0, 50, V).astype(np.int32)).to(ctx.device)
    n, d = ops.apply_bitmaps_owned(3, bits_all, levels, 9, visited, front, degrees)
    new = (parts[0] | parts[1] | parts[2]) & ~visited0
    own = np.zeros(V, bool); own[lo:hi] = True
    assert n == int((new & own).sum()) and d == int(degrees.cpu().numpy()[new & own].sum())
    assert np.array_equal(unpack(front), new) and np.array_equal(unpack(visited), visited0 | new)
    lv = levels.cpu().numpy()
    assert (lv[new & own] == 9).all() and (lv[~(new & own)] == -1).all()


def pagerank_exact_sums(O, rowptr, adj, iterations):
    """pr.hpp:37-136 with the reference's f32 expressions, except that every per-vertex sum of the f32 products is taken EXACTLY
    (f64 accumulation of < 2^20 f32 values is exact to ~1e-16) and rounded to f32 once -- what PR_BLOCKED computes."""
    V = len(rowptr) - 1
    indeg = O.indegree_noloops(rowptr, adj)
    rdeg = np.where(indeg == 0, 0.0, 1.0 / np.maximum(indeg, 1)).astype(np.float32)
    d = np.float32(0.85)
    k = np.float32((1.0 - np.float64(d)) / np.float64(np.float32(V)))
    ranks = np.full(V, np.float32(1.0 / V), np.float32)
    rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(rowptr))
    keep = rows != adj
    rows, cols = rows[keep], adj[keep]
    for _ in range(iterations):
        contrib = ranks * rdeg
        dangling = np.float32(np.sum((ranks[indeg == 0] / np.float32(V)).astype(np.float64)))
        acc = np.bincount(rows, weights=contrib[cols].astype(np.float64), minlength=V).astype(np.float32)
        ranks = k + d * (acc + dangling)
    return ranks


@pytest.mark.gpu
@pytest.mark.parametrize("kind,scale,ef,renumber", [("rmat", 12, 16, None), ("ru", 16, 8, None), ("rmat", 17, 16, "total"), ("rmat", 17, 16, None),
                                                    ("ru", 18, 4, None), ("ru", 15, 1, None)])
def test_pagerank_blocked_pull(kind, scale, ef, renumber, ctx, oracle):
    """PR_BLOCKED (LDS-window gather, exact 64-bit fixed-point sums, vgl_blocked.h): equal -- up to one f32 rounding -- to the
    restatement with exact per-vertex sums for ANY cut into units (so deterministic), and within 1e-6 relative (north star) of the
    oracle's adjacency-order f32 chain where rows are short (uniform inputs; on RMAT hubs the CHAIN is the inexact one).  One block,
    several blocks, blocks cut into several units (forced small units: slabs), self loops dropped at plan build time, zero iterations."""
    import os
    from vectorgraphlibrary_amd import api
    O = oracle
    V, seed = 1 << scale, 21
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    g = api.Graph.from_coo(ctx, V, src, dst, renumber=renumber)
    rowptr, adj = g.out_rowptr.cpu().numpy(), g.out_adj.cpu().numpy()
    for it in (0, 1, 4):
        ref_exact = pagerank_exact_sums(O, rowptr, adj, it)
        got = []
        for unit in ("", "64"):
            if unit:
                os.environ["VGL_BLK_GATHER_UNIT"] = os.environ["VGL_BLK_ACCUM_UNIT"] = unit
            try:
                g2 = api.Graph(ctx, V, g.out_rowptr, g.out_adj, g.in_rowptr, g.in_adj) if unit else g      # a fresh handle builds a fresh plan
                ranks, st = api.page_rank(g2, it, raw=True, mode=api.PR_BLOCKED)
            finally:
                os.environ.pop("VGL_BLK_GATHER_UNIT", None), os.environ.pop("VGL_BLK_ACCUM_UNIT", None)
            rk = ranks.cpu().numpy()
            got.append(rk)
            assert relerr(rk, ref_exact) <= 3e-7, (it, unit, relerr(rk, ref_exact))
            assert abs(st["ranks_sum"] - float(rk.astype(np.float64).sum())) < 1e-9
            if kind == "ru":
                assert relerr(rk, O.pagerank(rowptr, adj, it, 1)) <= PR_RTOL
            if unit:
                g2.close()
        assert (got[0].view(np.int32) == got[1].view(np.int32)).all(), "blocked sums depend on the cut into units"
    exact, _ = api.page_rank(g, 4, raw=True, mode=api.PR_EXACT_ORDER)
    assert (exact.cpu().numpy().view(np.int32) == O.pagerank(rowptr, adj, 4, 1).view(np.int32)).all()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,scale,ef,bound", [("ru", 16, 8, 1.0), ("rmat", 15, 16, 1.0), ("ru", 17, 4, 1000.0), ("ru", 14, 1, 0.3)])
def test_sum_over_edges_declared_operator(kind, scale, ef, bound, ctx, oracle):
    """vgl_hip_sum_over_edges_f32 (the declared operator VGL_SUM_OVER_EDGES; pull of algorithms/pr/pr.hpp:109-123 on the caller's arrays):
    sums[src] = sum of values[dst] over the edges src -> dst, dst != src, EXACT (f64 accumulation of f32 values is exact here) and rounded to
    f32 once, for any bound that covers the sums (the unit of the fixed point follows the bound) and for any cut into units."""
    import os
    import torch
    from vectorgraphlibrary_amd import api
    V, seed = 1 << scale, 77
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    g = api.Graph.from_coo(ctx, V, src, dst)
    rowptr, adj = g.out_rowptr.cpu().numpy(), g.out_adj.cpu().numpy()
    rng = np.random.default_rng(5)
    rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(rowptr))
    keep = rows != adj
    longest = int(np.diff(rowptr).max())
    values = (rng.random(V, dtype=np.float32) * np.float32(bound / max(longest, 1))).astype(np.float32)     # every sum stays below `bound`
    values[rng.integers(0, V, V // 16)] = 0.0
    want = np.bincount(rows[keep], weights=values[adj[keep]].astype(np.float64), minlength=V).astype(np.float32)
    x = torch.from_numpy(values).to(ctx.device)
    got = []
    for unit in ("", "64"):
        if unit:
            os.environ["VGL_BLK_GATHER_UNIT"] = os.environ["VGL_BLK_ACCUM_UNIT"] = unit
        try:
            g2 = api.Graph(ctx, V, g.out_rowptr, g.out_adj, g.in_rowptr, g.in_adj) if unit else g
            got.append(api.sum_over_edges(g2, x, bound).cpu().numpy())
        finally:
            os.environ.pop("VGL_BLK_GATHER_UNIT", None), os.environ.pop("VGL_BLK_ACCUM_UNIT", None)
        if unit:
            g2.close()
    assert (got[0].view(np.int32) == got[1].view(np.int32)).all(), "the sums depend on the cut into units"
    nz = want > 0
    # one f32 rounding of the exact sum; contributions below bound * 2^-62 are dropped by the fixed point (none here)
    assert np.max(np.abs(got[0][nz] - want[nz]) / want[nz]) <= 1.2e-7, np.max(np.abs(got[0][nz] - want[nz]) / want[nz])
    assert (got[0][~nz] == 0).all()
    with pytest.raises(Exception):
        api.sum_over_edges(g, x, 0.0)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,scale,ef,renumber", [("rmat", 17, 16, "total"), ("rmat", 17, 16, None), ("ru", 17, 8, None), ("ru", 16, 2, None)])
def test_sssp_pull_and_direction_optimising(kind, scale, ef, renumber, ctx, oracle):
    """pull (blocked gather / LDS minimum) and push <-> pull switching SSSP / SSWP on graphs of several blocks: f32 bits equal to the
    oracle's Bellman-Ford for every switch point (share 0: always pull after the first step; 2: never), reusable plan, small units
    (blocks cut into several units fold their minima with global atomics), several sources."""
    import os
    from vectorgraphlibrary_amd import api
    O = oracle
    V, seed = 1 << scale, 33
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    g = api.Graph.from_coo(ctx, V, src, dst, want_perm=True, renumber=renumber)
    w_d = ctx.gather_u32(g.perm, ctx.gen_weights(src.numel(), seed))
    rowptr, adj, w = g.out_rowptr.cpu().numpy(), g.out_adj.cpu().numpy(), w_d.cpu().numpy()
    # layouts: default (two-pass at these sizes), blocks cut into 64-chunk units, and dense block pairs as FUSED TILES -- forced down to
    # pairs of 64 edges, with 64-chunk pieces so that a pair is spread over several workgroups (what RMAT-24's hub pairs go through)
    # ... and the layout in row-range PIECES (what a direction with 2^32 edges or more gets), forced at a twentieth of the edges
    for unit, fuse, piece in (("", "", ""), ("64", "", ""), ("", "64", ""), ("64", "64", ""), ("", "", str(max(4096, src.numel() // 20))), ("", "64", str(max(4096, src.numel() // 7)))):
        if unit:
            os.environ["VGL_BLK_GATHER_UNIT"] = os.environ["VGL_BLK_ACCUM_UNIT"] = os.environ["VGL_BLK_FUSED_UNIT"] = unit
        if fuse:
            os.environ["VGL_BLK_FUSE_MIN"] = fuse
        if piece:
            os.environ["VGL_BLK_PIECE_EDGES"] = piece
        try:
            plan = api.SsspPullPlan(g, w_d)
        finally:
            for name in ("VGL_BLK_GATHER_UNIT", "VGL_BLK_ACCUM_UNIT", "VGL_BLK_FUSED_UNIT", "VGL_BLK_FUSE_MIN", "VGL_BLK_PIECE_EDGES"):
                os.environ.pop(name, None)
        assert plan.info()["edges"] == src.numel()
        for k in range(2):
            s = O.pick_source(rowptr, seed, k)
            ref, _ = O.sssp_bellman_ford(rowptr, adj, w, s)
            refw, _ = O.sswp_bellman_ford(rowptr, adj, w, s)
            for share in ("0", "0.35", "2"):
                os.environ["VGL_SSSP_PULL_SHARE"] = share
                try:
                    d, st = api.sssp(g, w_d, s, api.SSSP_DIRECTION_OPT, raw=True, plan=plan)
                    wd, wst = api.sswp(g, w_d, s, api.SSSP_DIRECTION_OPT, raw=True, plan=plan)
                finally:
                    del os.environ["VGL_SSSP_PULL_SHARE"]
                assert (d.cpu().numpy().view(np.int32) == ref.view(np.int32)).all(), (unit, fuse, piece, k, share)
                assert (wd.cpu().numpy().view(np.int32) == refw.view(np.int32)).all(), (unit, fuse, piece, k, share)
                assert st["push_steps"] + st["pull_steps"] == st["iterations"]
                if share == "2":
                    assert st["pull_steps"] == 0
            d, st = api.sssp(g, w_d, s, api.SSSP_PULL, raw=True, plan=plan)
            assert (d.cpu().numpy().view(np.int32) == ref.view(np.int32)).all() and st["push_steps"] == 0
        plan.close()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,scale,ef,piece", [("rmat", 16, 16, ""), ("ru", 15, 8, ""), ("rmat", 15, 16, "40000")])
def test_path_structure_is_built_once_per_graph_and_shared_between_weight_arrays(kind, scale, ef, piece, ctx, oracle):
    """Round 5 (the reference derives every edge-array layout from ONE permutation, csr_edges_array.hpp:31-40): the blocked layout of the path
    algorithms is a per-graph STRUCTURE that keeps the CSR position behind every value slot (vgl_hip_sssp_prepare) + per-weights value arrays filled
    by one gather pass.  Two plans with different weights share the structure and stay independent; a plan outlives the graph handle's own
    reference to the structure (a rebuild after a layout switch, the handle's close); and once the structure exists SSSP_ALL_ACTIVE -- the reference's schedule -- runs as blocked passes with the bits of
    the atomic push kernel (VGL_SSSP_ALL_ACTIVE_PUSH=1) and of the oracle."""
    import os
    from vectorgraphlibrary_amd import api
    O = oracle
    V, seed = 1 << scale, 91
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, seed)
    g = api.Graph.from_coo(ctx, V, src, dst, want_perm=True, renumber="total" if kind == "rmat" else None)
    rowptr, adj = g.out_rowptr.cpu().numpy(), g.out_adj.cpu().numpy()
    wa_d = ctx.gather_u32(g.perm, ctx.gen_weights(src.numel(), seed))
    wb_d = ctx.gather_u32(g.perm, ctx.gen_weights(src.numel(), seed + 1))
    wa, wb = wa_d.cpu().numpy(), wb_d.cpu().numpy()
    assert not np.array_equal(wa, wb)
    s = O.pick_source(rowptr, seed, 0)
    ref_a, _ = O.sssp_bellman_ford(rowptr, adj, wa, s)
    ref_b, _ = O.sssp_bellman_ford(rowptr, adj, wb, s)
    d0, st0 = api.sssp(g, wa_d, s, api.SSSP_ALL_ACTIVE, raw=True)                 # no structure yet: the atomic push kernel
    assert st0["pull_steps"] == 0 and (d0.cpu().numpy().view(np.int32) == ref_a.view(np.int32)).all()
    if piece:
        os.environ["VGL_BLK_PIECE_EDGES"] = piece                                 # the structure in row-range pieces (every piece keeps its own base)
    try:
        g.prepare_sssp()
        pa, pb = api.SsspPullPlan(g, wa_d), api.SsspPullPlan(g, wb_d)
        assert pa.info()["edges"] == src.numel() == pb.info()["edges"]
        for plan, w_d, ref in ((pa, wa_d, ref_a), (pb, wb_d, ref_b), (pa, wa_d, ref_a)):
            for mode in (api.SSSP_PULL, api.SSSP_DIRECTION_OPT):
                d, st = api.sssp(g, w_d, s, mode, raw=True, plan=plan)
                assert (d.cpu().numpy().view(np.int32) == ref.view(np.int32)).all(), mode
        d1, st1 = api.sssp(g, wb_d, s, api.SSSP_ALL_ACTIVE, raw=True)             # routed: blocked passes
        assert st1["pull_steps"] == st1["iterations"] > 0 and st1["push_steps"] == 0
        assert (d1.cpu().numpy().view(np.int32) == ref_b.view(np.int32)).all()
        os.environ["VGL_SSSP_ALL_ACTIVE_PUSH"] = "1"
        try:
            d2, st2 = api.sssp(g, wb_d, s, api.SSSP_ALL_ACTIVE, raw=True)
        finally:
            del os.environ["VGL_SSSP_ALL_ACTIVE_PUSH"]
        assert st2["pull_steps"] == 0 and (d2.cpu().numpy().view(np.int32) == ref_b.view(np.int32)).all()
        wd, _ = api.sswp(g, wa_d, s, api.SSSP_ALL_ACTIVE, raw=True)               # the widest-path algebra over the same structure
        assert (wd.cpu().numpy().view(np.int32) == O.sswp_bellman_ford(rowptr, adj, wa, s)[0].view(np.int32)).all()
        os.environ["VGL_BLK_FUSE_MIN"] = "64"                                     # a layout switch changed: the graph's structure is rebuilt ...
        try:
            pc = api.SsspPullPlan(g, wa_d)
        finally:
            del os.environ["VGL_BLK_FUSE_MIN"]
        for plan, w_d, ref in ((pa, wa_d, ref_a), (pb, wb_d, ref_b)):             # ... and the older plans keep theirs alive
            for mode in (api.SSSP_PULL, api.SSSP_DIRECTION_OPT):
                d, st = api.sssp(g, w_d, s, mode, raw=True, plan=plan)
                assert (d.cpu().numpy().view(np.int32) == ref.view(np.int32)).all(), mode
        pc.close()
    finally:
        os.environ.pop("VGL_BLK_PIECE_EDGES", None)
    pa.close()
    g.close()                                                                     # pb still holds the structure: it is freed with pb
    pb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,scale,ef,symmetric", [("rmat", 16, 8, True), ("ru", 17, 2, True), ("rmat", 16, 8, False), ("ru", 15, 1, False)])
def test_cc_blocked_hook(kind, scale, ef, symmetric, ctx, oracle):
    """Shiloach-Vishkin with the hook as a blocked pass (vgl_blocked.h, forced on at these sizes): labels equal to the oracle's on symmetric
    and on directed inputs (min id that reaches each vertex), whole-graph run and three shards driven in lock-step, small units."""
    import os
    import torch
    from vectorgraphlibrary_amd import api
    import protocol_model as vd
    O = oracle
    g, V, hs, hd, rowptr, adj, perm = build_case(ctx, O, kind, scale, ef, 17, symmetric=symmetric)
    ref, _ = O.cc_sv(rowptr, adj)
    # layouts: default (dense pairs of 16384-id blocks become fused tiles from 16384 edges: most pairs of these graphs), everything two-pass,
    # and both with 64-chunk units / pieces
    for unit, fuse, piece in (("", "", ""), ("64", "", ""), ("", "0", ""), ("64", "0", ""), ("64", "64", ""), ("", "", "50000"), ("64", "0", "30000")):
        os.environ["VGL_CC_BLOCKED"] = "1"
        if unit:
            os.environ["VGL_BLK_GATHER_UNIT"] = os.environ["VGL_BLK_ACCUM_UNIT"] = os.environ["VGL_BLK_FUSED_UNIT"] = unit
        if fuse:
            os.environ["VGL_BLK_FUSE_MIN"] = fuse
        if piece:
            os.environ["VGL_BLK_PIECE_EDGES"] = piece             # row-range pieces, as for a direction with 2^32 edges or more
        try:
            g2 = api.Graph(ctx, V, g.out_rowptr, g.out_adj, g.in_rowptr, g.in_adj)
            comp, st = api.connected_components(g2)
            assert (comp.cpu().numpy() == ref).all(), (unit, fuse, "whole graph")
            bounds = ctx.partition_rows(g.out_rowptr, 3)
            shards = [g.shard(bounds[p], bounds[p + 1]) for p in range(3)]
            comps = torch.arange(V, dtype=torch.int32, device=ctx.device)
            while True:                                                      # lock-step: every shard hooks its rows into the shared labels
                changed = 0
                for s in shards:
                    changed |= vd.HipShardOps(s).cc_hook(comps)
                if not changed:
                    break
                vd.HipShardOps(shards[0]).cc_jump(comps)
            assert (comps.cpu().numpy() == ref).all(), (unit, "shards")
            for s in shards:
                s.close()
            g2.close()
        finally:
            for k in ("VGL_CC_BLOCKED", "VGL_BLK_GATHER_UNIT", "VGL_BLK_ACCUM_UNIT", "VGL_BLK_FUSED_UNIT", "VGL_BLK_FUSE_MIN", "VGL_BLK_PIECE_EDGES"):
                os.environ.pop(k, None)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(12))
def test_random_graphs_blocked_paths(seed, ctx, oracle):
    """differential sweep of the blocked advance (vgl_blocked.h) over random graphs of awkward shapes -- V below, at and above one
    32768-vertex block and not a multiple of anything, empty graphs, isolated vertices, self loops, duplicates, hub rows -- with the
    default and with tiny work units (every block cut in many units: slabs, global-atomic folds): SSSP / SSWP pull and
    direction-optimising, Shiloach-Vishkin with the blocked hook, PageRank with exact sums, all against the oracle"""
    import os
    import torch
    from vectorgraphlibrary_amd import api
    O = oracle
    rng = np.random.default_rng(7000 + seed)
    V = [1, 63, 4097, 32767, 32768, 32769, 50001, 70000, 98305, 140001][seed % 10]
    E = int(rng.integers(0, 6 * V + 1)) if seed % 6 else 0
    src = np.minimum((rng.random(E) ** (1 + seed % 3) * V).astype(np.int32), V - 1)
    dst = np.minimum((rng.random(E) ** (1 + (seed // 3) % 3) * V).astype(np.int32), V - 1)
    rowptr, adj, perm = O.coo_to_csr(V, src, dst)
    w_in = (rng.random(E) * 100).astype(np.float32)
    w = w_in[perm] if E else np.zeros(0, np.float32)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device) if len(a) else torch.zeros(0, dtype=dt, device=ctx.device)
    source = int(rng.integers(0, V))
    ref_dist, _ = O.sssp_bellman_ford(rowptr, adj, w, source)
    ref_width, _ = O.sswp_bellman_ford(rowptr, adj, w, source)
    ref_comp = O.cc_sv(rowptr, adj)[0]
    ref_pr = pagerank_exact_sums(O, rowptr, adj, 3)
    ref_levels, ref_bst = O.bfs_top_down(rowptr, adj, source)
    for unit in ("", "64"):
        os.environ["VGL_CC_BLOCKED"] = "1"
        if unit:
            os.environ["VGL_BLK_GATHER_UNIT"] = os.environ["VGL_BLK_ACCUM_UNIT"] = unit
        try:
            g = api.Graph.from_coo(ctx, V, dev(src, torch.int32), dev(dst, torch.int32), want_perm=True)
            w_d = ctx.gather_u32(g.perm, dev(w_in, torch.float32)) if E else torch.zeros(1, dtype=torch.float32, device=ctx.device)
            for mode in (api.SSSP_PULL, api.SSSP_DIRECTION_OPT):
                d, st = api.sssp(g, w_d, source, mode)
                assert (d.cpu().numpy().view(np.int32) == ref_dist.view(np.int32)).all(), (unit, mode)
                wd, _ = api.sswp(g, w_d, source, mode)
                assert (wd.cpu().numpy().view(np.int32) == ref_width.view(np.int32)).all(), (unit, mode)
            assert (api.connected_components(g)[0].cpu().numpy() == ref_comp).all(), unit
            rk = api.page_rank(g, 3, mode=api.PR_BLOCKED)[0].cpu().numpy()
            assert relerr(rk, ref_pr) <= 3e-7, (unit, relerr(rk, ref_pr))
            # blocked top-down levels: every level (share 0), the default rule, and never -- same levels and statistics
            g.prepare_blocked_bfs()
            for share in ("0", "", "2"):
                if share:
                    os.environ["VGL_BFS_BLOCKED_SHARE"] = share
                for bmode in (api.BFS_TOP_DOWN, api.BFS_DIRECTION_OPT):
                    lv, bst = api.bfs(g, source, bmode)
                    assert (lv.cpu().numpy() == ref_levels).all(), (unit, share, bmode)
                    assert bst["discovered"] == ref_bst["discovered"] and bst["frontier_total"] == ref_bst["frontier_total"]
                    if bmode == api.BFS_TOP_DOWN:
                        assert bst["edges_examined"] == ref_bst["edges_examined"] and bst["levels"] == ref_bst["levels"]
                os.environ.pop("VGL_BFS_BLOCKED_SHARE", None)
            g.close()
        finally:
            for k in ("VGL_CC_BLOCKED", "VGL_BLK_GATHER_UNIT", "VGL_BLK_ACCUM_UNIT", "VGL_BFS_BLOCKED_SHARE"):
                os.environ.pop(k, None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,scale,ef", [("rmat", 16, 32), ("uniform", 15, 16), ("rmat", 18, 32)])
def test_bfs_blocked_top_down_levels(kind, scale, ef, ctx, oracle):
    """vgl_hip_bfs_prepare_blocked: top-down traversals whose large levels run as the blocked pass (one bit per edge through LDS windows)
    return the levels, level count and work statistics of the plain top-down run and of the oracle (bfs.hpp:6-51); degree-renumbered and
    identity numbering, several sources, share 0 (every level blocked) and the default rule"""
    import os
    import torch
    from vectorgraphlibrary_amd import api
    O = oracle
    V = 1 << scale
    hs, hd = (O.gen_rmat if kind == "rmat" else O.gen_uniform)(scale, ef, 3)
    rowptr, adj, _ = O.coo_to_csr(V, hs, hd)
    s_d, d_d = torch.from_numpy(hs).to(ctx.device), torch.from_numpy(hd).to(ctx.device)
    for renumber in (None, "total"):
        g = api.Graph.from_coo(ctx, V, s_d, d_d, renumber=renumber)
        plain = {}
        srcs = [int(x) for x in np.nonzero(np.diff(rowptr) > 0)[0][[1, 77, 4321]]]
        for s in srcs:
            plain[s] = api.bfs(g, s, api.BFS_TOP_DOWN)
        g.prepare_blocked_bfs()
        try:
            for share in ("", "0"):
                if share:
                    os.environ["VGL_BFS_BLOCKED_SHARE"] = share
                for s in srcs:
                    ref, ref_st = O.bfs_top_down(rowptr, adj, s)
                    lv, st = api.bfs(g, s, api.BFS_TOP_DOWN)
                    assert (lv.cpu().numpy() == ref).all(), (renumber, share, s)
                    assert torch.equal(lv, plain[s][0])
                    for k in ("levels", "edges_examined", "frontier_total", "discovered"):
                        assert st[k] == ref_st[k] == plain[s][1][k], (k, renumber, share, s)
                    lv2, _ = api.bfs(g, s, api.BFS_DIRECTION_OPT)
                    assert (lv2.cpu().numpy() == ref).all()
        finally:
            os.environ.pop("VGL_BFS_BLOCKED_SHARE", None)
        g.close()
