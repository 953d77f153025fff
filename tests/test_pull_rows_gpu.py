"""vgl_k_pull_sum (vgl_pull.h) on rows placed by hand (tests/pull_rows_graphs.py; what the rows are is proved in tests/test_pull_rows_cpu.py):
PageRank's ordered f32 chain against the oracle bit for bit -- ordinary rows, hub wavefronts, giant workgroups, under every switch that moves a
row from one path to another, on shards, and with in-degrees crafted so that a lost entry or a changed order changes the bits -- and the chunked
f64 sums of HITS against the oracle at the project's 1e-12."""
import contextlib
import os

import numpy as np
import pytest

import pull_rows_graphs as P
from test_gpu_parity import HITS_RTOL, _relerr64, pagerank_exact_sums, relerr

ITERATIONS = (1, 3)


@contextlib.contextmanager
def _switches(env):
    """the switches are read when a graph's hub lists are built: set around the creation of a fresh handle and its first run"""
    os.environ.update(env)
    try:
        yield
    finally:
        for name in env:
            os.environ.pop(name, None)


class _Ladder:
    def __init__(self, ctx, O):
        import torch
        from vectorgraphlibrary_amd import api
        self.ctx, self.O, self.api = ctx, O, api
        self.V, src, dst, self.rows = P.ladder()
        self.rowptr, self.adj, _ = O.coo_to_csr(self.V, src, dst)
        self.g = api.Graph.from_coo(ctx, self.V, torch.from_numpy(src).to(ctx.device), torch.from_numpy(dst).to(ctx.device))
        self.crafted = P.crafted_indeg(self.V, P.under_test(self.rows))
        self.d_crafted = torch.from_numpy(self.crafted).to(ctx.device)
        self._want = {}

    def fresh(self, with_incoming=True):
        g = self.g
        return self.api.Graph(self.ctx, self.V, g.out_rowptr, g.out_adj, *((g.in_rowptr, g.in_adj) if with_incoming else ()))

    def want(self, crafted, it):
        """the oracle's ranks, computed once per (in-degrees, iterations) and never written to"""
        if (crafted, it) not in self._want:
            r = self.O.pagerank(self.rowptr, self.adj, it, 1, indeg=self.crafted if crafted else None)
            r.setflags(write=False)
            self._want[(crafted, it)] = r
        return self._want[(crafted, it)]

    def check_bits(self, got, want, what):
        got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
        bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
        if bad.size:
            v = int(bad[0])
            pytest.fail("%s: %d of %d vertices differ; first: vertex %d, row of %d entries, case %s, got %r, want %r" % (
                what, bad.size, self.V, v, int(self.rowptr[v + 1] - self.rowptr[v]), "/".join(P.case_of(self.rows, v)), got[v], want[v]))

    def run_exact(self, g, crafted, what):
        for it in ITERATIONS:
            ranks, _ = self.api.page_rank(g, it, indeg_noloops=self.d_crafted if crafted else None, raw=True, mode=self.api.PR_EXACT_ORDER)
            self.check_bits(ranks, self.want(crafted, it), "%s, %d iterations" % (what, it))


@pytest.fixture(scope="module")
def ladder(ctx, oracle):
    lad = _Ladder(ctx, oracle)
    yield lad
    lad.g.close()


@pytest.mark.gpu
def test_device_csr_keeps_input_order(ladder):
    """adjacency order within a row = input order (the stable build): what makes the ladder's positions the kernel's positions"""
    g = ladder.g
    assert (g.out_rowptr.cpu().numpy() == ladder.rowptr).all() and (g.out_adj.cpu().numpy() == ladder.adj).all()
    in_rowptr, in_adj = ladder.O.transpose_csr(ladder.rowptr, ladder.adj)
    assert (g.in_rowptr.cpu().numpy() == in_rowptr).all() and (g.in_adj.cpu().numpy() == in_adj).all()


@pytest.mark.gpu
def test_pagerank_ladder_default_switches(ladder):
    """default thresholds (the 32768+ rows are giants): crafted in-degrees, and the graph's own through both in-degree kernels"""
    ladder.run_exact(ladder.g, True, "crafted in-degrees")
    ladder.run_exact(ladder.g, False, "in-degrees from the incoming CSR minus self loops")
    out_only = ladder.fresh(with_incoming=False)
    try:
        ladder.run_exact(out_only, False, "in-degrees by per-edge atomics")
    finally:
        out_only.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,value", [("VGL_PULL_HUB_BLOCKS", "1"), ("VGL_PULL_GIANT_DEGREE", "513"), ("VGL_PULL_GIANT_DEGREE", "1025"),
                                        ("VGL_PULL_NO_GIANTS", "1")])
def test_pagerank_ladder_switches(name, value, ladder):
    """one hub workgroup (4 wavefronts own all hubs, longest first); every hub but the 512-entry ones a giant (more giants than giant workgroups,
    2 .. 7 batches); giants from 1025 entries; no giants at all (the 40000-entry row on one wavefront)"""
    with _switches({name: value}):
        g = ladder.fresh()
        try:
            ladder.run_exact(g, True, "%s=%s" % (name, value))
        finally:
            g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"VGL_PULL_GIANT_DEGREE": "513"}], ids=["default", "giant513"])
@pytest.mark.parametrize("name", sorted(P.SMALL))
def test_small_graphs(name, env, ctx, oracle):
    import torch
    from vectorgraphlibrary_amd import api
    V, src, dst = P.SMALL[name]()
    rowptr, adj, _ = oracle.coo_to_csr(V, src, dst)
    d_src, d_dst = torch.from_numpy(src).to(ctx.device), torch.from_numpy(dst).to(ctx.device)
    for with_incoming in (True, False):
        with _switches(env):
            g = api.Graph.from_coo(ctx, V, d_src, d_dst, with_incoming=with_incoming)
            try:
                assert (g.out_adj.cpu().numpy() == adj).all()
                for it in ITERATIONS:
                    ranks, _ = api.page_rank(g, it, raw=True, mode=api.PR_EXACT_ORDER)
                    want = oracle.pagerank(rowptr, adj, it, 1)
                    assert (ranks.cpu().numpy().view(np.int32) == want.view(np.int32)).all(), (name, it, with_incoming, ranks.cpu().numpy(), want)
                if with_incoming:
                    wa, wh = oracle.hits(rowptr, adj, 2)
                    a, h = api.hits(g, 2)
                    assert _relerr64(a.cpu().numpy(), wa) <= HITS_RTOL and _relerr64(h.cpu().numpy(), wh) <= HITS_RTOL
            finally:
                g.close()


@pytest.mark.gpu
def test_pagerank_ladder_shards(ladder):
    """three row ranges; the middle one has row_begin > 0, starts with a hub (its first block opens inside the hub's entries) and owns the long
    rows with self loops (self = row_base + r in all three paths)"""
    from protocol_model import HipShardOps
    bounds = P.SHARD_BOUNDS
    shards = [ladder.g.shard(bounds[p], bounds[p + 1]) for p in range(3)]
    try:
        ops = [HipShardOps(s) for s in shards]
        ranks, rdeg, contrib = ops[0].new_f32(), ops[0].new_f32(), ops[0].new_f32()
        ops[0].pr_setup(ladder.d_crafted, ranks, rdeg)
        for _ in range(2):
            new = [ranks.clone() for _ in ops]
            for p, o in enumerate(ops):
                o.pr_iteration(ladder.d_crafted, rdeg, new[p], contrib)
            for p in range(3):
                ranks[bounds[p]:bounds[p + 1]] = new[p][bounds[p]:bounds[p + 1]]
        ladder.check_bits(ranks, ladder.want(True, 2), "3 shards, 2 iterations")
    finally:
        for s in shards:
            s.close()


@pytest.mark.gpu
def test_pagerank_ladder_blocked(ladder):
    """PR_BLOCKED on the same rows: exact fixed-point sums, the same bits for any cut into units, one f32 rounding from the restatement"""
    api = ladder.api
    for it in ITERATIONS:
        ref = pagerank_exact_sums(ladder.O, ladder.rowptr, ladder.adj, it)
        got = []
        for unit in ("", "64"):
            with _switches({"VGL_BLK_GATHER_UNIT": unit, "VGL_BLK_ACCUM_UNIT": unit} if unit else {}):
                g = ladder.fresh()
                try:
                    ranks, _ = api.page_rank(g, it, raw=True, mode=api.PR_BLOCKED)
                    got.append(ranks.cpu().numpy())
                finally:
                    g.close()
            print("blocked, %d iterations, unit %r: relative error %.3g" % (it, unit, relerr(got[-1], ref)))
            assert relerr(got[-1], ref) <= 3e-7, (it, unit, relerr(got[-1], ref))
        ladder.check_bits(got[0], got[1], "blocked sums depend on the cut into units, %d iterations" % it)


@pytest.mark.gpu
def test_hits_ladder(ladder):
    """in-rows of 512 .. 12289 entries (1 .. 4 chunks, 267 chunks: the last chunk workgroup is partly idle; 260 hubs: two finish workgroups),
    out-rows up to 40000 entries; the unordered path sizes its own grid, so VGL_PULL_HUB_BLOCKS must not matter"""
    import torch
    api = ladder.api
    wa, wh = ladder.O.hits(ladder.rowptr, ladder.adj, 2)
    a, h = api.hits(ladder.g, 2)
    ea, eh = _relerr64(a.cpu().numpy(), wa), _relerr64(h.cpu().numpy(), wh)
    print("hits, 2 steps: relative error auth %.3g, hub %.3g" % (ea, eh))
    assert ea <= HITS_RTOL and eh <= HITS_RTOL, (ea, eh)
    a2, h2 = api.hits(ladder.g, 2)
    assert torch.equal(a2, a) and torch.equal(h2, h)
    a0, h0 = api.hits(ladder.g, 0)
    assert float(a0.min()) == 1.0 == float(a0.max()) and float(h0.min()) == 1.0 == float(h0.max())
    with _switches({"VGL_PULL_HUB_BLOCKS": "1"}):
        g = ladder.fresh()
        try:
            a3, h3 = api.hits(g, 2)
        finally:
            g.close()
    assert torch.equal(a3, a) and torch.equal(h3, h)
