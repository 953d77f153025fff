"""Betweenness centrality at full size.  RMAT-20 x 16 (16.8 M stored entries), 8 sources, against the numpy / scipy restatement with the derived tolerance
of tests/test_bc_gpu.py.  RMAT-24 x 32 (537 M stored entries, the BASELINE BFS graph), 4 sources: no scipy matrix of that size is built; every source is
checked by the certificate that needs no reference (the sum of its dependencies is an integer given by its levels), by its levels being those of
api.bfs, and the whole call by running it twice (bit-identical) and by the sum of the per-source dependencies (the source's own left out)."""
import numpy as np
import pytest
import torch

import bc_reference as R

pytestmark = pytest.mark.gpu


def test_bc_rmat20_against_the_restatement(ctx):
    from vectorgraphlibrary_amd import api
    scale, ef, V = 20, 16, 1 << 20
    src, dst = ctx.gen_rmat(scale, ef, 1)
    s_np, d_np = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
    outdeg = np.bincount(s_np, minlength=V)
    sources = [0] + np.flatnonzero(outdeg > 0)[1000:1007].tolist()
    g = api.Graph.from_coo(ctx, V, src, dst, renumber="total")
    ref, info = R.betweenness(V, s_np, d_np, sources)
    got, st = api.betweenness_centrality(g, sources, want_last=True)
    tol = R.tolerance(info["max_depth"], info["d_max"], len(sources))
    print({k: v for k, v in st.items() if not torch.is_tensor(v)}, "D", info["max_depth"], "d_max", info["d_max"], "sigma max", info["sigma_max"])
    ok, frac = R.compare(got.cpu().numpy(), ref, tol)
    print("RMAT-20 largest error / bound %.4f (bound %.3e relative)" % (frac, tol))
    assert ok, frac
    for k in ("sources", "max_depth", "levels_total", "reached_total", "edges_forward", "edges_backward"):
        assert st[k] == info[k], (k, st[k], info[k])
    levels, sigma, _ = info["last"]
    assert info["sigma_max"] < 2.0 ** 53 and st["sigma_inexact"] == 0
    assert np.array_equal(st["levels"].cpu().numpy(), levels) and np.array_equal(st["sigma"].cpu().numpy(), sigma)
    g.close()


def test_bc_rmat24_by_certificate_levels_and_reproducibility(ctx):
    from vectorgraphlibrary_amd import api
    scale, ef, V = 24, 32, 1 << 24
    src, dst = ctx.gen_rmat(scale, ef, 1)
    g = api.Graph.from_coo(ctx, V, src, dst, renumber="total")
    del src, dst
    torch.cuda.empty_cache()
    g.prepare_betweenness()
    deg = g.out_rowptr[1:] - g.out_rowptr[:-1]
    d_max = int(max(int(deg.max()), int((g.in_rowptr[1:] - g.in_rowptr[:-1]).max())))
    sources = [0] + torch.nonzero(deg > 0).flatten()[100000:100003].tolist()        # the graph's own numbering: vertex 0 is the heaviest hub
    del deg
    total = torch.zeros(V, dtype=torch.float64, device=ctx.device)
    for s in sources:
        one, st = api.betweenness_centrality(g, [s], raw=True, want_last=True)
        levels, _ = api.bfs(g, s, raw=True)
        assert torch.equal(st["levels"], levels)
        want = int((levels[levels > 1].to(torch.int64) - 2).sum())                   # R.certificate on the device
        got = float(st["delta"].sum() - st["delta"][s])
        tol = R.tolerance(st["max_depth"], d_max, 1) + V * R.U
        print("source", s, {k: v for k, v in st.items() if not torch.is_tensor(v)}, "certificate", got, "expected", want, "error / bound %.4f" % (abs(got - want) / (tol * want)))
        assert st["reached_total"] == int((levels > 0).sum()) and st["max_depth"] == int(levels.max()) - 1
        assert abs(got - want) <= tol * want
        assert float(st["sigma"][s]) == 1.0 and bool(((st["sigma"] > 0) == (levels > 0)).all())
        assert float(one[s]) == 0.0 and bool((one >= 0).all())
        total += one
        del one, st, levels
    a, st_a = api.betweenness_centrality(g, sources, raw=True)
    b, _ = api.betweenness_centrality(g, sources, raw=True)
    assert torch.equal(a, b)                                                         # bit-identical
    ok, frac = R.compare(a.cpu().numpy(), total.cpu().numpy(), R.tolerance(st_a["max_depth"], d_max, len(sources)))
    print("RMAT-24 one call against the sum of single-source calls: error / bound %.4f" % frac, {k: v for k, v in st_a.items()})
    assert ok, frac
    g.close()
