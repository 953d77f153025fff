"""The 12-byte head records of the bottom-up BFS step (VGL_BFS_HEADS=auto|wide|packed, read when a graph handle is created; four 24-bit ids per
record, 0xFFFFFF = absent; chosen only when every id that occurs in a record is below 0xFFFFFF) against the 16-byte int4 records: on every graph
below direction-optimising BFS from several sources gives the levels of oracle.bfs_top_down and the SAME statistics record with either form, and
at least one traversal per graph runs bottom-up steps (so vgl_k_bu_probe ran on the records under test).

Whether a source turns bottom-up is worked out on the CPU from the oracle's levels and the switch rule (`turns_bottom_up`: F > previous F and
M >= ((V - visited) * factor + V) / 15, change_state.hpp) and asserted before anything runs on the GPU, so the condition does not depend on the
form under test.  The id-width boundary graph has ~3 M edges instead of a few hundred thousand for that reason: with V = 2^24 the rule needs a
frontier of at least 2 V / 15 = 2.2 M out-edges before any level can turn bottom-up."""
import os
import threading
import uuid

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STATS = ("levels", "edges_examined", "frontier_total", "discovered", "td_steps", "bu_steps", "bu_edges", "bu_found")
ALPHA = 15


class heads:
    """VGL_BFS_HEADS for the graph handles created inside the block"""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = os.environ.get("VGL_BFS_HEADS")
        if self.form is None:
            os.environ.pop("VGL_BFS_HEADS", None)
        else:
            os.environ["VGL_BFS_HEADS"] = self.form

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("VGL_BFS_HEADS", None)
        else:
            os.environ["VGL_BFS_HEADS"] = self.old


def turns_bottom_up(rowptr, levels):
    """the switch rule on the oracle's levels: does some level of this traversal turn bottom-up?"""
    V = len(rowptr) - 1
    E = int(rowptr[-1])
    factor = max(E // V // 2, 1)
    deg = np.diff(rowptr)
    prev_f, visited = 0, 0
    for lv in range(int(levels.max()) + 1):
        members = levels == lv
        f, m = int(members.sum()), int(deg[members].sum())
        visited += f
        if f > prev_f and m >= ((V - visited) * factor + V) // ALPHA:
            return True
        prev_f = f
    return False


def host_csr(g):
    return g.out_rowptr.cpu().numpy(), g.out_adj.cpu().numpy()


def check_forms(ctx, oracle, make_graph, sources, expect_wide="wide", expect_packed="packed"):
    """make_graph() under VGL_BFS_HEADS=wide and =packed: levels of the oracle and identical statistics from every source (the graph's own
    numbering), bottom-up steps in at least one run; returns the oracle's levels per source"""
    from vectorgraphlibrary_amd import api
    with heads("wide"):
        gw = make_graph()
    with heads("packed"):
        gp = make_graph()
    assert gw.info()["bfs_heads"] == expect_wide and gp.info()["bfs_heads"] == expect_packed
    assert gw.info()["in_nz_rows"] == gp.info()["in_nz_rows"]
    rowptr, adj = host_csr(gw)
    refs = {s: oracle.bfs_top_down(rowptr, adj, s)[0] for s in sources}
    assert any(turns_bottom_up(rowptr, refs[s]) for s in sources), "no source of this graph turns bottom-up: the probe kernel would not run"
    bu_steps = 0
    for s in sources:
        lw, sw = api.bfs(gw, s, api.BFS_DIRECTION_OPT, raw=True)
        lp, sp = api.bfs(gp, s, api.BFS_DIRECTION_OPT, raw=True)
        assert (lw.cpu().numpy() == refs[s]).all(), ("wide", s)
        assert (lp.cpu().numpy() == refs[s]).all(), ("packed", s)
        assert {k: sw[k] for k in STATS} == {k: sp[k] for k in STATS}, s
        bu_steps += sw["bu_steps"]
    assert bu_steps > 0
    gw.close()
    gp.close()
    return refs


def kinds_of_sources(rowptr, in_rowptr):
    """a hub, a leaf, a vertex without incoming edges (that has outgoing ones) and a vertex without outgoing edges"""
    out_deg, in_deg = np.diff(rowptr), np.diff(in_rowptr)
    return [int(np.argmax(out_deg)), int(np.nonzero(out_deg == 1)[0][0]), int(np.nonzero((in_deg == 0) & (out_deg > 0))[0][0]),
            int(np.nonzero(out_deg == 0)[0][0])]


@pytest.mark.parametrize("scale", [12, 14])
@pytest.mark.parametrize("renumber", ["total", None])
def test_rmat_multigraph_levels_and_stats_equal(ctx, oracle, scale, renumber):
    """RMAT keeps its duplicate edges: a duplicate in-neighbour is stored once per record (the records hold DISTINCT ids) and must not be read as
    padding -- the statistics count the probes a sequential scan of the record would have made"""
    from vectorgraphlibrary_amd import api
    V = 1 << scale
    src, dst = ctx.gen_rmat(scale, 16, 7)

    def make():
        return api.Graph.from_coo(ctx, V, src, dst, renumber=renumber)
    with heads("wide"):
        g = make()
    sources = kinds_of_sources(g.out_rowptr.cpu().numpy(), g.in_rowptr.cpu().numpy())
    g.close()
    check_forms(ctx, oracle, make, sources)


# ---- the hand-built graph: every decode lane, the absent-entry field in every position, the hand-over to the deferred pass ----
HAND_V = 4096
HAND_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 300)
LOW = range(1, 1000)            # fillers below the frontier's ids: no incoming edges, so never visited from vertex 0
FRONT = range(1000, 1064)       # level 1 of the traversal from vertex 0: the frontier the bottom-up level probes against
HIGH = range(2000, 3000)        # fillers above the frontier's ids
FIRST_TARGET = 3000


def hand_graph():
    """Vertex 0 points at the 64 vertices of FRONT; they point at 20 `bulk` rows each (enough out-edges for the rule to turn level 1 bottom-up).
    A target row of n in-edges with its only frontier in-neighbour at position k of its ascending ids has k - 1 fillers from LOW and n - k from
    HIGH; position 0 = no frontier in-neighbour at all (the row stays unreached).  Returns src, dst and {target: (n, k)}."""
    src, dst, rows = [], [], {}
    t = FIRST_TARGET
    for i, f in enumerate(FRONT):
        src.append(0)
        dst.append(f)
    for n in HAND_LENGTHS:
        for k in sorted(set(range(0, min(n, 10) + 1)) | {n}):
            low = [LOW[(7 * t + j) % len(LOW)] for j in range(max(k - 1, 0))] if k else []
            high_n = n - k if k else n
            high = [HIGH[(11 * t + j) % len(HIGH)] for j in range(high_n)]
            ins = low + ([FRONT[t % len(FRONT)]] if k else []) + high
            assert len(set(ins)) == n
            for u in ins:
                src.append(u)
                dst.append(t)
            rows[t] = (n, k)
            t += 1
    bulk0 = t
    for i, f in enumerate(FRONT):
        for j in range(20):
            src.append(f)
            dst.append(bulk0 + (i * 20 + j) % (HAND_V - 1 - bulk0))
    # a second level behind the targets: the found ones point at a row that the NEXT bottom-up (or top-down) level has to find
    for tt, (n, k) in rows.items():
        if k:
            src.append(tt)
            dst.append(HAND_V - 1)
    return np.array(src, np.int32), np.array(dst, np.int32), rows


def test_hand_built_rows_every_head_position(ctx, oracle):
    from vectorgraphlibrary_amd import api
    src_np, dst_np, rows = hand_graph()
    in_deg = np.bincount(dst_np, minlength=HAND_V)
    for t, (n, k) in rows.items():
        assert in_deg[t] == n
    assert {n for n, _ in rows.values()} >= {1, 3, 4, 5, 7, 8, 9, 16, 300}
    for want in ((8, 4), (8, 5), (8, 8), (9, 9), (16, 10), (16, 16), (300, 300), (8, 0), (9, 0), (300, 0), (4, 4), (5, 5)):
        assert want in rows.values()            # only the 4th / 5th / 8th head, beyond the heads, none (in_long clear and set)
    src, dst = torch.from_numpy(src_np).to(ctx.device), torch.from_numpy(dst_np).to(ctx.device)

    def make():
        return api.Graph.from_coo(ctx, HAND_V, src, dst)
    filler = int(src_np[(src_np > 0) & (src_np < FRONT[0])][0])
    # the hub; a leaf (a found row: one edge, to the last vertex); a filler (no incoming edges); rows without outgoing edges; a frontier vertex
    sources = [0, FIRST_TARGET + 1, filler, FIRST_TARGET, HAND_V - 1, FRONT[3]]
    assert rows[FIRST_TARGET] == (1, 0) and rows[FIRST_TARGET + 1] == (1, 1)
    refs = check_forms(ctx, oracle, make, sources)
    lv = refs[0]
    for t, (n, k) in rows.items():
        assert lv[t] == (3 if k else -1), (t, n, k)                # (the source is level 1)
    assert lv[HAND_V - 1] == 4


# ---- the id-width boundary ----
B_V = 1 << 24
B_TOP = B_V - 2                 # the largest id the packed form can hold


def boundary_edges(V, extra=()):
    """vertex 0 -> 300 frontier vertices (B_TOP among them) -> 10 000 pseudo-random rows each (3 M edges: see the module docstring), a row
    of B_TOP's points back into the graph, plus `extra` edges"""
    rng = np.random.default_rng(24)
    front = np.unique(np.concatenate([rng.integers(1, B_V - 2, 299), [B_TOP]])).astype(np.int64)
    src = [np.zeros(len(front), np.int64)]
    dst = [front]
    for f in front:
        src.append(np.full(10000, f, np.int64))
        dst.append(rng.integers(1, B_TOP - 1, 10000))
    far = dst[-1][:50]
    src.append(far)
    dst.append(np.full(50, B_TOP - 1, np.int64))               # edges INTO a neighbour id of the boundary, from rows B_TOP found
    for u, v in extra:
        src.append(np.array([u], np.int64))
        dst.append(np.array([v], np.int64))
    return np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32)


def _levels_ok(ctx, oracle, g, source=0):
    from vectorgraphlibrary_amd import api
    rowptr, adj = host_csr(g)
    ref = oracle.bfs_top_down(rowptr, adj, source)[0]
    lv, st = api.bfs(g, source, api.BFS_DIRECTION_OPT, raw=True)
    assert (lv.cpu().numpy() == ref).all()
    return ref, st


def test_id_width_boundary_packs_up_to_the_last_id_but_one(ctx, oracle):
    from vectorgraphlibrary_amd import api
    src_np, dst_np = boundary_edges(B_V)
    assert (src_np == B_TOP).any() and (dst_np == B_TOP).any() and not (src_np == B_V - 1).any()
    src, dst = torch.from_numpy(src_np).to(ctx.device), torch.from_numpy(dst_np).to(ctx.device)

    def make():
        return api.Graph.from_coo(ctx, B_V, src, dst)
    refs = check_forms(ctx, oracle, make, [0])
    assert refs[0][B_TOP] == 2 and refs[0][B_TOP - 1] == 4      # (the source is level 1)
    with heads(None):
        g = make()
    assert g.info()["bfs_heads"] == "packed"                   # auto
    ref, st = _levels_ok(ctx, oracle, g)
    assert st["bu_steps"] > 0
    g.close()


@pytest.mark.parametrize("form", [None, "packed"])
def test_id_width_boundary_last_id_as_in_neighbour_stays_wide(ctx, oracle, form):
    """one edge whose source is vertex 2^24 - 1 = the absent-entry field: the records stay wide under auto and under `packed`"""
    from vectorgraphlibrary_amd import api
    src_np, dst_np = boundary_edges(B_V)
    target = int(dst_np[1000])
    src_np, dst_np = boundary_edges(B_V, extra=[(B_V - 1, target)])
    src, dst = torch.from_numpy(src_np).to(ctx.device), torch.from_numpy(dst_np).to(ctx.device)
    with heads(form):
        g = api.Graph.from_coo(ctx, B_V, src, dst)
    assert g.info()["bfs_heads"] == "wide"
    ref, st = _levels_ok(ctx, oracle, g)
    assert st["bu_steps"] > 0 and ref[target] == 3 and ref[B_V - 1] == -1
    g.close()


def test_ids_beyond_24_bits_stay_wide(ctx, oracle):
    from vectorgraphlibrary_amd import api
    V = B_V + 64
    src_np, dst_np = boundary_edges(V, extra=[(V - 1, 5)])
    src, dst = torch.from_numpy(src_np).to(ctx.device), torch.from_numpy(dst_np).to(ctx.device)
    with heads(None):
        g = api.Graph.from_coo(ctx, V, src, dst)
    assert g.info()["bfs_heads"] == "wide"
    _, st = _levels_ok(ctx, oracle, g)
    assert st["bu_steps"] > 0
    g.close()


# ---- record addressing at the tail of a plane ----
def test_ragged_sizes_v_not_a_multiple_of_64_records_not_of_4(ctx, oracle):
    from vectorgraphlibrary_amd import api
    V = 5003
    rng = np.random.default_rng(3)
    src_np = (V * rng.random(16 * V) ** 3).astype(np.int32)       # skewed: hubs at the low ids, rows with one and with no outgoing edge
    dst_np = rng.integers(0, V - 1, 16 * V).astype(np.int32)        # (the last vertex has no incoming edge)
    keep = (dst_np % 7 != 3) & (src_np % 11 != 5)                   # a seventh of the rows has no record at all, an eleventh no outgoing edge
    src_np, dst_np = src_np[keep], dst_np[keep]
    nz_rows = len(np.unique(dst_np))
    assert V % 64 != 0 and nz_rows % 4 != 0
    src, dst = torch.from_numpy(src_np).to(ctx.device), torch.from_numpy(dst_np).to(ctx.device)

    def make():
        return api.Graph.from_coo(ctx, V, src, dst)
    with heads("wide"):
        g = make()
    assert g.info()["in_nz_rows"] == nz_rows
    sources = kinds_of_sources(g.out_rowptr.cpu().numpy(), g.in_rowptr.cpu().numpy()) + [V - 1]
    g.close()
    check_forms(ctx, oracle, make, sources)


# ---- shards hold global ids and share the kernel ----
def test_two_hosted_ranks_on_one_gpu_with_packed_heads_equal_fused(ctx):
    """two ranks as threads of this process over the hosted transport, scale 14, shards created under VGL_BFS_HEADS=packed: levels bit-identical to
    the fused traversal (wide records) of the whole graph.  The ranks are threads, as in test_sharded_bfs_eight_rank_threads_one_gpu of
    tests/test_sharded_gpu.py, and not that file's _run_ranks processes: its helper script is fixed at scale 13 and runs all five drivers (tens of
    seconds); this runs the BFS alone at the size asked for and can ask every shard for the form of its records."""
    from vectorgraphlibrary_amd import api
    from vectorgraphlibrary_amd import sharded as vs
    scale, ef, seed, world = 14, 16, 5, 2
    V, E = 1 << scale, (1 << scale) * ef
    src, dst = ctx.gen_rmat(scale, ef, seed)
    with heads("wide"):
        g = api.Graph.from_coo(ctx, V, src, dst, renumber="total")
    deg = g.out_rowptr[1:] - g.out_rowptr[:-1]
    sources = [int(torch.argmax(deg)), int(torch.nonzero(deg == 1)[0])]
    fused = [api.bfs(g, s, api.BFS_DIRECTION_OPT, raw=True) for s in sources]
    assert sum(st["bu_steps"] for _, st in fused) > 0
    bounds = ctx.partition_rows(g.out_rowptr, world)
    pieces = []
    for r in range(world):
        sh = g.shard(bounds[r], bounds[r + 1])
        pieces.append((sh.out_rowptr, sh.out_adj, sh.in_rowptr, sh.in_adj, bounds[r], bounds[r + 1]))
        sh.close()
    ctx.sync()
    name = "/vgl_pk_%s" % uuid.uuid4().hex[:12]
    errors, forms, bu_steps = [], [], []

    def rank_main(r):
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=0)):
                c = api.Context(0)
                orp, oadj, irp, iadj, lo, hi = pieces[r]
                sh = api.Graph(c, V, orp, oadj, irp, iadj, lo, hi)
                forms.append(sh.info()["bfs_heads"])
                comm = vs.Comm.hosted(c, r, world, name, slot_bytes=1 << 16)
                for s, (ref, _) in zip(sources, fused):
                    lv, st = vs.bfs_run_sharded(sh, comm, s, api.BFS_DIRECTION_OPT, global_edges=E, gather_levels=True)
                    assert torch.equal(lv, ref), (r, s)
                    bu_steps.append(st["bu_steps"])
                comm.barrier()
                comm.close()
                sh.close()
                c.close()
        except Exception as e:                         # noqa: BLE001
            errors.append((r, repr(e)))

    with heads("packed"):
        threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errors, errors
    assert forms == ["packed"] * world and sum(bu_steps) > 0    # ids of a scale-14 graph fit: the shards did probe packed records
    g.close()
