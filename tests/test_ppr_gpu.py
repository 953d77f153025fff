"""Batched personalised PageRank on the GPU (vgl_hip_ppr_run, api.personalized_pagerank / pagerank, apps/bin/ppr_hip) against the numpy / scipy
restatement of the contract (tests/ppr_reference.py) on ORIGINAL ids.  Two float64 evaluations are compared within twice the derived tolerance
(ppr_reference.tolerance); supports, p itself, determinism and the integer stats are compared for equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ppr_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = ["ppr_pull_short", "ppr_pull_wave", "ppr_pull_wg", "ppr_fold", "ppr_teleport", "ppr_out"]
SHRUNK = {"VGL_PPR_SHORT": "4", "VGL_PPR_WAVE": "16", "VGL_PPR_CHUNK": "64"}


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def coo(ctx, src, dst):
    return (torch.tensor(np.asarray(src, dtype=np.int32), device=ctx.device), torch.tensor(np.asarray(dst, dtype=np.int32), device=ctx.device))


def bits(t):
    return t.contiguous().view(torch.int64)


def l1(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).sum())


def problems(V, count, seed):
    """count seed lists and their weights: single seeds, a repeated source, lists of several weighted seeds, a vertex listed twice, the empty list"""
    rng = np.random.default_rng(seed)
    lists, weights = [], []
    for j in range(count):
        kind = j % 6
        if kind in (0, 3):
            lists.append([int(rng.integers(0, V))]); weights.append([1.0])
        elif kind == 1:
            lists.append([7 % V]); weights.append([2.5])                    # the same source again and again
        elif kind == 2:
            k = int(rng.integers(2, 6))
            lists.append([int(v) for v in rng.integers(0, V, k)]); weights.append([float(w) for w in rng.uniform(0.1, 4.0, k)])
        elif kind == 4:
            a, b = int(rng.integers(0, V)), int(rng.integers(0, V))
            lists.append([a, b, a]); weights.append([1.0, 2.0, 0.5])        # a listed twice
        else:
            lists.append([]); weights.append([])
    return lists, weights


def check(g, G, lists, weights, alpha, t, what, **kw):
    """one API call with tol = 0 against the restatement: every column within twice the tolerance, of mass 1 and not negative; the integer stats"""
    A = api()
    rank, info = A.personalized_pagerank(g, lists, weights, alpha=alpha, max_iterations=t, with_stats=True, **kw)
    want, _, _, st = R.pagerank(G, lists, weights, alpha, t)
    got = rank.cpu().numpy()
    tol = R.tolerance(G.d_max, G.n_dangling, alpha, t)
    assert rank.dtype == torch.float64 and got.shape == (len(lists), G.V)
    worst = max([l1(got[j], want[j]) for j in range(len(lists))], default=0.0)
    print(what, "alpha", alpha, "t", t, "largest L1 difference", worst, "bound", 2 * tol)
    assert worst <= 2 * tol, what
    assert (got >= 0).all(), what
    for j in range(len(lists)):
        assert abs(float(got[j].sum()) - 1.0) <= tol + G.V * R.U, (what, j)
    for k in ("sources", "batches", "iterations_total", "iterations_max", "entries_walked"):
        assert info[k] == st[k], (what, k, info[k], st[k])
    assert info["batches_converged"] == 0 and info["iterations"].tolist() == [t] * len(lists)
    return rank, info, want


@pytest.fixture(scope="module")
def graphs(ctx):
    """name -> (restatement graph, handle): the fixed small graphs, RMAT-10 x 8 as it is and renumbered by out-degree"""
    A = api()
    out = {}
    for name in R.SMALL:
        V, src, dst = R.small(name)
        out[name] = (R.Graph(V, src, dst), A.Graph.from_coo(ctx, V, *coo(ctx, src, dst)))
    V = 1 << 10
    src, dst = ctx.gen_rmat(10, 8, 2)
    G = R.Graph(V, src.cpu().numpy(), dst.cpu().numpy())
    out["rmat10"] = (G, A.Graph.from_coo(ctx, V, src, dst))
    out["rmat10_renumbered"] = (G, A.Graph.from_coo(ctx, V, src, dst, renumber="out"))
    yield out
    for _, g in out.values():
        g.close()


@pytest.mark.parametrize("alpha", [0.5, 0.85])
@pytest.mark.parametrize("t", [1, 3, 50])
def test_fixed_iterations(t, alpha, graphs):
    for name, (G, g) in graphs.items():
        lists, weights = problems(G.V, 6, 3)
        check(g, G, lists, weights, alpha, t, name)


def test_renumbered_graph_speaks_original_ids(graphs):
    A = api()
    G, g = graphs["rmat10_renumbered"]
    _, plain = graphs["rmat10"]
    assert g.fwd is not None
    lists, weights = problems(G.V, 6, 5)
    a = A.personalized_pagerank(g, lists, weights, max_iterations=10).cpu().numpy()
    b = A.personalized_pagerank(plain, lists, weights, max_iterations=10).cpu().numpy()
    tol = R.tolerance(G.d_max, G.n_dangling, 0.85, 10)
    assert max(l1(a[j], b[j]) for j in range(6)) <= 2 * tol
    raw = A.personalized_pagerank(g, [[g.vertex_id(v) for v in s] for s in lists], weights, max_iterations=10, raw=True)
    assert torch.equal(bits(raw[:, g.fwd.long()]), bits(torch.tensor(a, device=raw.device)))


def test_support_and_p_by_equality(graphs):
    """t = 3: rank != 0 exactly on the restatement's support, 0.0 elsewhere: a column that leaks into its neighbour shows here.  alpha = 0 and t = 0
    return p bit for bit."""
    A = api()
    for name, (G, g) in graphs.items():
        lists, weights = problems(G.V, 17, 11)
        rank = A.personalized_pagerank(g, lists, weights, alpha=0.85, max_iterations=3).cpu().numpy()
        p = np.stack([R.teleport(G.V, s, w) for s, w in zip(lists, weights)])
        for j, s in enumerate(lists):
            if s:
                assert np.array_equal(rank[j] != 0, R.support(G, s, 3)), (name, j)
            else:
                assert (rank[j] > 0).all(), (name, j)
        for kw in ({"alpha": 0.0, "max_iterations": 4}, {"alpha": 0.85, "max_iterations": 0}):
            got, info = A.personalized_pagerank(g, lists, weights, with_stats=True, **kw)
            assert np.array_equal(got.cpu().numpy().view(np.int64), p.view(np.int64)), (name, kw)
            if kw["max_iterations"] == 0:
                assert info["err"].tolist() == [0.0] * 17 and info["iterations"].tolist() == [0] * 17 and info["entries_walked"] == 0


def launches(ctx):
    return {k: ctx.timing_get(k)[0] for k in SLOTS}


def test_row_lengths_and_every_class(ctx, monkeypatch):
    """incoming rows of 0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 1023, 1024 and 1025 entries: at the default bounds, then with the bounds shrunk so that
    every class and several chunks per row are walked"""
    A = api()
    V, src, dst = R.row_length_graph()
    G = R.Graph(V, src, dst)
    assert sorted(set(G.indeg.tolist())) == [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025]
    lists, weights = problems(V, 17, 13)
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    ctx.timing(True)
    first, info, _ = check(g, G, lists, weights, 0.85, 4, "row lengths, default bounds")
    n = launches(ctx)
    ctx.timing(False)
    print("launches", n)
    assert info["prepared_now"] == 1 and n["ppr_pull_short"] > 0 and n["ppr_pull_wave"] > 0 and n["ppr_pull_wg"] > 0
    g.close()
    for k, v in SHRUNK.items():
        monkeypatch.setenv(k, v)
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))                       # a new handle under the shrunk switches
    ctx.timing(True)
    for count in (1, 3, 17):
        got, _, _ = check(g, G, lists[:count], weights[:count], 0.85, 4, "row lengths, shrunk bounds, %d" % count)
        tol = R.tolerance(G.d_max, G.n_dangling, 0.85, 4)
        assert max(l1(got[j].cpu().numpy(), first[j].cpu().numpy()) for j in range(count)) <= 2 * tol
    n = launches(ctx)
    ctx.timing(False)
    print("launches", n)
    assert all(v > 0 for v in n.values()), n
    g.close()


def test_in_star_above_the_chunk(ctx):
    """40 000 leaves point at the centre: one row above the default chunk, cut into three.  Uniform p: by symmetry every leaf holds l and the centre
    (dangling) c, with  l' = (alpha c + 1 - alpha) / V,  c' = alpha n l + (alpha c + 1 - alpha) / V."""
    A = api()
    n, t, alpha = 40000, 5, 0.85
    V = n + 1
    src, dst = np.arange(1, V), np.zeros(n, dtype=np.int64)
    g = A.Graph.from_coo(ctx, V, *coo(ctx, src, dst))
    ctx.timing(True)
    rank, info = A.personalized_pagerank(g, [[], [1]], alpha=alpha, max_iterations=t, with_stats=True)
    wg = ctx.timing_get("ppr_pull_wg")[0]
    ctx.timing(False)
    assert wg == 2 * t                                                      # the chunks, then the one writer per long row
    leaf = c = 1.0 / V
    for _ in range(t):
        tele = (alpha * c + (1.0 - alpha)) / V
        leaf, c = tele, alpha * (n * leaf) + tele
    tol = R.tolerance(n, 1, alpha, t)
    got = rank.cpu().numpy()
    print("centre", got[0, 0], "closed form", c, "bound", 2 * tol * c)
    assert abs(got[0, 0] - c) <= 2 * tol and abs(got[0, 1:] - leaf).sum() <= 2 * tol
    assert len(set(got[0, 1:].tolist())) == 1
    # the listed column: leaf 1 and the centre alone
    assert np.array_equal(got[1] != 0, np.arange(V) <= 1) and abs(got[1].sum() - 1.0) <= tol + V * R.U
    assert info["entries_walked"] == t * n
    g.close()


@pytest.mark.parametrize("count", [1, 2, 15, 16, 17, 33])
def test_batch_shapes(count, graphs):
    G, g = graphs["rmat10"]
    lists, weights = problems(G.V, 33, 17)
    assert any(not s for s in lists[:15]) and any(len(s) == 3 and s[0] == s[2] for s in lists[:15])
    check(g, G, lists[:count], weights[:count], 0.85, 5, "%d problems" % count)


def test_position_and_width_agree_within_the_tolerance(graphs):
    A = api()
    G, g = graphs["rmat10"]
    s, t = [3], 20
    fill = [[v] for v in range(40, 72)]
    alone = A.personalized_pagerank(g, [s], max_iterations=t)[0]
    shapes = {"width 4, place 2": (fill[:2] + [s], 2), "width 16, place 5": (fill[:5] + [s] + fill[5:12], 5), "second batch, width 1": (fill[:16] + [s], 16),
              "second batch, width 4, place 1": (fill[:17] + [s] + fill[17:18], 17)}
    tol = R.tolerance(G.d_max, G.n_dangling, 0.85, t)
    for what, (lists, at) in shapes.items():
        got = A.personalized_pagerank(g, lists, max_iterations=t)[at]
        d = float((got - alone).abs().sum())
        print(what, "L1 to the single run", d, "bound", 2 * tol)
        assert d <= 2 * tol, what


def test_dangling_everything_and_nothing(graphs):
    """all of the seeds' mass reaches dangling vertices in one step; and two graphs without a dangling vertex"""
    G, g = graphs["all_dangling_after_one_step"]
    assert G.dangling[4:].all() and not G.dangling[:4].any()
    rank, _, want = check(g, G, [[0], [1, 2], [3, 0]], [[1.0], [1.0, 3.0], [2.0, 2.0]], 0.85, 2, "all dangling")
    one = api().personalized_pagerank(g, [[0]], max_iterations=1)[0].cpu().numpy()
    assert one[4] == 0.85 and one[0] == 1.0 - 0.85 and one[[1, 2, 3, 5, 6]].sum() == 0.0      # nothing has come back yet
    for name in ("cycle_directed", "complete"):
        G, g = graphs[name]
        assert G.n_dangling == 0
        check(g, G, [[0], [], [1, 2]], [[1.0], [], [1.0, 1.0]], 0.85, 30, name)


def test_same_call_same_bits(graphs):
    A = api()
    G, g = graphs["rmat10"]
    lists, weights = problems(G.V, 33, 19)
    one, a = A.personalized_pagerank(g, lists, weights, max_iterations=20, with_stats=True)
    two, b = A.personalized_pagerank(g, lists, weights, max_iterations=20, with_stats=True)
    assert torch.equal(bits(one), bits(two)) and torch.equal(bits(a["err"]), bits(b["err"]))
    assert a["prepared_now"] == 0 and b["prepared_now"] == 0 and a["max_err"] == b["max_err"] == float(a["err"].max())


def test_tolerance_mode(graphs):
    A = api()
    G, g = graphs["rmat10"]
    lists, weights = problems(G.V, 20, 23)
    tol, cap = 1e-8, 500
    rank, info = A.personalized_pagerank(g, lists, weights, max_iterations=cap, tol=tol, with_stats=True)
    err, its = info["err"].cpu().numpy(), info["iterations"].cpu().numpy()
    print("iterations", its.tolist(), "err", err.tolist())
    converged = 0
    for base in (0, 16):
        members = slice(base, min(base + 16, 20))
        assert len(set(its[members].tolist())) == 1
        assert err[members].max() <= tol or its[base] == cap
        converged += int(err[members].max() <= tol)
    assert info["batches_converged"] == converged == 2 and info["iterations_total"] == int(its[0]) + int(its[16]) and info["iterations_max"] == its.max()
    assert info["entries_walked"] == info["iterations_total"] * G.E and info["max_err"] == err.max()
    got = rank.cpu().numpy()
    for j in (0, 2, 5, 19):
        star = R.dense_solve(G, R.teleport(G.V, lists[j], weights[j]), 0.85)
        d, bound = l1(got[j], star), 0.85 * err[j] / 0.15 + R.tolerance(G.d_max, G.n_dangling, 0.85, int(its[j]))
        print("problem", j, "L1 to the dense solve", d, "bound", bound)
        assert d <= bound
    # a tolerance out of reach: the cap stops the batch
    rank, info = A.personalized_pagerank(g, lists[:3], weights[:3], max_iterations=5, tol=1e-30, with_stats=True)
    assert info["iterations"].tolist() == [5] * 3 and info["batches_converged"] == 0 and float(info["err"].min()) > 1e-30


def test_symmetric_without_incoming_csr(ctx):
    A = api()
    V = 1 << 10
    src, dst = ctx.gen_rmat(10, 8, 7)
    both = (torch.cat([src, dst]), torch.cat([dst, src]))
    G = R.Graph(V, both[0].cpu().numpy(), both[1].cpu().numpy())
    lists, weights = problems(V, 6, 29)
    with_in = A.Graph.from_coo(ctx, V, *both)
    no_in = A.Graph.from_coo(ctx, V, *both, with_incoming=False)
    a, _, _ = check(with_in, G, lists, weights, 0.85, 10, "symmetrised, incoming CSR")
    b, _, _ = check(no_in, G, lists, weights, 0.85, 10, "symmetrised, outgoing CSR only", symmetric=True)
    tol = R.tolerance(G.d_max, G.n_dangling, 0.85, 10)
    assert float((a - b).abs().sum(dim=1).max()) <= 2 * tol
    no_in.prepare_ppr(symmetric=True)
    for h in (with_in, no_in):
        h.close()


def test_pagerank_is_the_empty_list(graphs):
    A = api()
    G, g = graphs["rmat10"]
    pr = A.pagerank(g)
    col, info = A.personalized_pagerank(g, [[]], tol=1e-10, with_stats=True)
    assert pr.shape == (G.V,) and torch.equal(bits(pr), bits(col[0])) and info["batches"] == 1
    star = R.dense_solve(G, R.teleport(G.V, []), 0.85)
    assert l1(pr.cpu().numpy(), star) <= 0.85 * float(info["err"][0]) / 0.15 + R.tolerance(G.d_max, G.n_dangling, 0.85, int(info["iterations"][0]))


def raw_run(ctx, g, seeds, ptr, weights, rank, count=None, alpha=0.85, iters=3, tol=0.0, symmetric=0):
    A = api()
    c_s = (C.c_int32 * max(len(seeds), 1))(*seeds)
    c_p = (C.c_int64 * len(ptr))(*ptr)
    c_w = None if weights is None else (C.c_double * max(len(weights), 1))(*weights)
    st = A._l.PprStats()
    A._l.check(ctx.L.vgl_hip_ppr_run(ctx.h, g.h, c_s, c_p, c_w, len(ptr) - 1 if count is None else count, alpha, iters, tol, symmetric,
                                     None if rank is None else C.c_void_p(rank.data_ptr()), None, None, C.byref(st)))
    ctx.sync()
    return st


def test_refusals_leave_the_output_untouched(ctx, graphs):
    A = api()
    G, g = graphs["rmat10"]
    V = G.V
    src, dst = ctx.gen_rmat(10, 8, 2)
    no_in = A.Graph.from_coo(ctx, V, src, dst, with_incoming=False)
    sh = g.shard(0, V // 2)
    rank = torch.full((2 * V,), -7.0, dtype=torch.float64, device=ctx.device)
    untouched = lambda: bool((rank == -7.0).all())
    nan, inf = float("nan"), float("inf")
    cases = [(dict(g=sh), "own all rows"), (dict(g=sh, symmetric=1), "own all rows"), (dict(g=no_in), "incoming CSR"),
             (dict(alpha=1.0), "alpha"), (dict(alpha=-0.1), "alpha"), (dict(alpha=nan), "alpha"), (dict(alpha=inf), "alpha"),
             (dict(tol=-1e-9), "tol"), (dict(tol=nan), "tol"), (dict(tol=inf), "tol"), (dict(iters=-1), "max_iterations"), (dict(count=-1), "count"),
             (dict(ptr=[0, 2, 1]), "seed_ptr"), (dict(seeds=[0, V]), "out of range"), (dict(seeds=[-1, 0]), "out of range"),
             (dict(weights=[1.0, 0.0]), "weight"), (dict(weights=[1.0, -2.0]), "weight"), (dict(weights=[nan, 1.0]), "weight"), (dict(weights=[inf, 1.0]), "weight")]
    for kw, message in cases:
        a = dict(g=g, seeds=[0, 1], ptr=[0, 1, 2], weights=None)
        a.update(kw)
        with pytest.raises(A._l.VglHipError, match=message):
            raw_run(ctx, a.pop("g"), a.pop("seeds"), a.pop("ptr"), a.pop("weights"), rank, **a)
        assert untouched(), (kw, message)
    with pytest.raises(A._l.VglHipError, match="d_rank"):
        raw_run(ctx, g, [0, 1], [0, 1, 2], None, None)
    with pytest.raises(A._l.VglHipError, match="incoming CSR"):
        no_in.prepare_ppr()
    with pytest.raises(A._l.VglHipError, match="own all rows"):
        sh.prepare_ppr()
    st = raw_run(ctx, g, [], [0], None, rank)                               # count == 0 succeeds and writes nothing
    assert st.sources == 0 and st.batches == 0 and untouched()
    st = raw_run(ctx, g, [0, 1], [0, 1, 2], None, rank)
    assert st.sources == 2 and st.batches == 1 and st.iterations_total == 3 and st.entries_walked == 3 * G.E and not bool((rank == -7.0).any())
    for h in (sh, no_in):
        h.close()


def test_ppr_app():
    cmd = [os.path.join(ROOT, "apps", "bin", "ppr_hip"), "-gen", "-s", "10", "-e", "8", "-fused", "-sources", "20", "-check"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "error count: 0" in out.stdout and "AVG_PERF" in out.stdout and "PPR launches:" in out.stdout, out.stdout
