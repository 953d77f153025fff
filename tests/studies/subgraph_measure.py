#!/usr/bin/env python3
"""What DESIGN section 24 quotes for subgraph extraction and neighbour sampling (GPU box).  Per graph, five workloads: the induced 16-core, a random
half vertex mask, the 2-hop ego graph of 1024 seeds, and fanout 10 and 25 for 2^20 seeds.  For each: the time of the library call (the median of 5
after one warm-up call, host clock around a call that ends in a device synchronise; masks, core numbers and seeds are prepared outside), the split
into plan and fill from the event brackets of a run of its own, the fill kernels' share of the HBM peak on the fill's part of algorithmic_bytes, and
NEXT TO IT the time of what a user does without these entry points: torch boolean indexing of the CSR plus Graph.from_coo (two key sorts) for the
subgraphs, and a torch sort of (row, key) for the samples.  Nothing here gates anything: nobody had measured this path.
usage: python3 tests/studies/subgraph_measure.py OUT.json [kind:scale:edge_factor ...]    (default rmat:20:16)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from vectorgraphlibrary_amd import api

PLAN_SLOTS = ["sub_scan", "sub_count_short", "sub_count_wave", "sub_count_wg", "sub_publish"]
FILL_SLOTS = ["sub_fill_short", "sub_fill_wave", "sub_fill_wg"]
SAMPLE_SLOTS = ["sample_count", "sample_publish", "sample_short", "sample_wave", "sample_wg"]
HBM_PEAK = 8.0e12
REPS = 5
SEEDS_EGO = 1024
SEEDS_SAMPLE = 1 << 20


def timed(call):
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        del out
    return {"ms": [round(t, 3) for t in times], "ms_median": round(statistics.median(times), 3)}


def slots(ctx, call, names):
    ctx.timing(True)
    out = call()
    torch.cuda.synchronize()
    r = {k: {"launches": ctx.timing_get(k)[0], "ms": round(ctx.timing_get(k)[1], 4)} for k in names}
    ctx.timing(False)
    return r, out


def torch_induced(g, keep):
    """the parent commit's path: boolean indexing of the CSR, then from_coo (keep: bool [V] in the graph's own numbering)"""
    deg = g.out_rowptr[1:] - g.out_rowptr[:-1]
    src = torch.repeat_interleave(torch.arange(g.V, device=keep.device, dtype=torch.int32), deg)
    m = keep[src.long()] & keep[g.out_adj.long()]
    new_id = (torch.cumsum(keep, 0) - 1).to(torch.int32)
    return api.Graph.from_coo(g.ctx, int(keep.sum()), new_id[src[m].long()], new_id[g.out_adj[m].long()])


def torch_sample(g, seeds, fanout, seed):
    """the same selection with torch: every entry of the seeds' rows, a sort by (row, key), the first fanout of a row, back in ascending position"""
    s = seeds.long()
    start, deg = g.out_rowptr[s], g.out_rowptr[s + 1] - g.out_rowptr[s]
    row = torch.repeat_interleave(torch.arange(s.numel(), device=s.device), deg)
    first = torch.cumsum(deg, 0) - deg
    pos = start[row] + (torch.arange(row.numel(), device=s.device) - first[row])
    order = torch.argsort((row << 32) | api.priority_key(pos, seed))
    rank = torch.arange(row.numel(), device=s.device) - first[row[order]]
    chosen = torch.sort(order[rank < fanout]).values
    return g.out_adj[pos[chosen]]


def subgraph_workload(ctx, g, keep_u8):
    call = lambda: api._row_filter(g, keep_u8, None, None, False, True, "measure")
    r = {"library": timed(call), "torch_indexing_plus_from_coo": timed(lambda: torch_induced(g, keep_u8.bool()))}
    kern, sub = slots(ctx, call, PLAN_SLOTS + FILL_SLOTS)
    st = sub.stats
    r["stats"], r["kernels"] = st, kern
    r["plan_kernels_ms"] = round(sum(kern[k]["ms"] for k in PLAN_SLOTS), 4)
    r["fill_kernels_ms"] = round(sum(kern[k]["ms"] for k in FILL_SLOTS), 4)
    vk = st["vertices_kept"]
    fill_bytes = sum(28 * vk + 16 * (vk + 1) + 8 * st["entries_read_" + d] + 4 * st["entries_kept_" + d] for d in ("out", "in"))
    r["fill_bytes"] = fill_bytes
    r["fill_share_of_hbm_peak"] = round(fill_bytes / max(r["fill_kernels_ms"] * 1e-3, 1e-9) / HBM_PEAK, 5)
    r["speedup"] = round(r["torch_indexing_plus_from_coo"]["ms_median"] / r["library"]["ms_median"], 2)
    return r


def sample_workload(ctx, g, seeds, fanout):
    call = lambda: api._sample_raw(g, seeds, int(seeds.numel()), fanout, 1, "out", False)
    r = {"library": timed(call), "torch_sort": timed(lambda: torch_sample(g, seeds, fanout, 1))}
    kern, out = slots(ctx, call, SAMPLE_SLOTS)
    assert torch.equal(out[1], torch_sample(g, seeds, fanout, 1)), "the torch selection differs"
    r["stats"], r["kernels"] = out[3], kern
    emit = sum(kern[k]["ms"] for k in SAMPLE_SLOTS[2:])
    r["emit_kernels_ms"] = round(emit, 4)
    r["share_of_hbm_peak"] = round(out[3]["algorithmic_bytes"] / (r["library"]["ms_median"] * 1e-3) / HBM_PEAK, 5)
    r["speedup"] = round(r["torch_sort"]["ms_median"] / r["library"]["ms_median"], 2)
    return r


def measure(ctx, kind, scale, ef):
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, 1)
    t0 = time.perf_counter()
    g = api.Graph.from_coo(ctx, V, src, dst)
    torch.cuda.synchronize()
    row = {"graph": "%s-%dx%d" % (kind, scale, ef), "V": V, "E": g.E, "from_coo_ms": round((time.perf_counter() - t0) * 1e3, 3)}
    del src, dst
    print(json.dumps(row), flush=True)
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)

    keep = api.k_core(g, 16, raw=True).to(torch.uint8)
    row["induced_16_core"] = subgraph_workload(ctx, g, keep)
    print(json.dumps(row["induced_16_core"]), flush=True)
    keep = (torch.rand(V, device=ctx.device, generator=gen) < 0.5).to(torch.uint8)
    row["random_half_mask"] = subgraph_workload(ctx, g, keep)
    print(json.dumps(row["random_half_mask"]), flush=True)

    seeds = torch.randint(0, V, (SEEDS_EGO,), dtype=torch.int32, device=ctx.device, generator=gen)
    row["k_hop_2"] = timed(lambda: api._k_hop_raw(g, seeds, SEEDS_EGO, 2, "out", False))
    hop, st = api._k_hop_raw(g, seeds, SEEDS_EGO, 2, "out", False)
    row["k_hop_2"]["stats"] = st
    row["ego_2_hop"] = subgraph_workload(ctx, g, (hop >= 0).to(torch.uint8))
    print(json.dumps(row["ego_2_hop"]), flush=True)
    del hop, keep
    torch.cuda.empty_cache()

    seeds = torch.randint(0, V, (SEEDS_SAMPLE,), dtype=torch.int32, device=ctx.device, generator=gen)
    for fanout in (10, 25):
        row["sample_fanout_%d" % fanout] = sample_workload(ctx, g, seeds, fanout)
        print(json.dumps(row["sample_fanout_%d" % fanout]), flush=True)
    return row


def main():
    args = sys.argv[1:]
    out = args.pop(0)
    graphs = args or ["rmat:20:16"]
    ctx = api.Context(0)
    rows = []
    for spec in graphs:
        kind, scale, ef = spec.split(":")
        rows.append(measure(ctx, kind, int(scale), int(ef)))
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
