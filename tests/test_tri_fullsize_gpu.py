"""Triangle counting at full size: the symmetrised RMAT-24 x 16 (537 M stored entries, the CC configuration of test_gpu_fullsize.py).  No CPU
reference exists at that size; instead properties that a wrong kernel breaks: sum(per_vertex) == 3 * triangles, per_vertex[v] <= d (d - 1) / 2, the
count and the per-vertex counts equal between renumber=None and renumber="total" (another orientation, another class split, the same answer), and
the count equal with and without the per-vertex counts."""
import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 1


def test_tri_rmat24_symmetrised(ctx):
    from vectorgraphlibrary_amd import api
    V = 1 << 24
    results = {}
    for renumber in (None, "total"):
        s, d = ctx.gen_rmat(24, 16, SEED)
        s, d = torch.cat([s, d]), torch.cat([d, s])
        g = api.Graph.from_coo(ctx, V, s, d, with_incoming=False, renumber=renumber)
        del s, d
        g.prepare_triangle_count()
        T0, st0 = api.triangle_count(g)
        T, st = api.triangle_count(g, clustering=True)
        print("renumber", renumber, "triangles", T, {k: v for k, v in st.items() if not torch.is_tensor(v)})
        assert T0 == T and T > 0 and st0["prepared_now"] == 0
        t, deg = st["per_vertex"], st["degree"].to(torch.int64)
        assert int(t.sum()) == 3 * T
        assert bool((t <= deg * (deg - 1) // 2).all()) and bool((t >= 0).all())
        assert int(deg.sum()) == 2 * st["undirected_edges"]
        assert float(st["clustering"].max()) <= 1.0
        results[renumber] = (T, t.cpu(), st["degree"].cpu(), st["undirected_edges"])
        g.close()
        del g, t, deg, st
        torch.cuda.empty_cache()
    a, b = results[None], results["total"]
    assert a[0] == b[0] and a[3] == b[3]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
