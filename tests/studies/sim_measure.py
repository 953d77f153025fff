#!/usr/bin/env python3
"""What DESIGN section 23 quotes for vertex similarity and link prediction (GPU box): the prepare time, and for three workloads -- the common
neighbours of ALL undirected edges, of 10^7 random pairs, and the top-10 Jaccard candidates of 4096 queries (the first vertices with a neighbour) --
the time of a call (the median of 5 after one warm-up call, host clock around a call that ends in a device synchronise), the per-slot split from a
run of its own with the event brackets on, the per-class rows, scratch_slots, and the bytes model of include/vgl_hip.h over the run time as a share
of the HBM peak.  The edge list comes from maximal_matching() outside every timing.  Nothing here gates anything: nobody had measured this path.
usage: python3 tests/studies/sim_measure.py OUT.json [kind:scale:edge_factor ...]    (default rmat:20:16)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from vectorgraphlibrary_amd import api

PAIR_SLOTS = ["sim_classify", "sim_publish", "sim_pairs_short", "sim_pairs_wave", "sim_pairs_wg"]
TOPK_SLOTS = ["sim_classify", "sim_publish", "sim_topk_small", "sim_topk_table", "sim_topk_global"]
HBM_PEAK = 8.0e12
REPS = 5
RANDOM_PAIRS = 10 ** 7
QUERIES = 4096


def timed(call):
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        st = call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times, st


def workload(ctx, call, slots):
    times, st = timed(call)
    r = {"run_ms": [round(t, 3) for t in times], "run_ms_median": round(statistics.median(times), 3),
         "stats": {k: v for k, v in st.items() if not torch.is_tensor(v)}}
    r["share_of_hbm_peak"] = round(st["algorithmic_bytes"] / (r["run_ms_median"] * 1e-3) / HBM_PEAK, 5)
    ctx.timing(True)
    call()
    torch.cuda.synchronize()
    r["kernels"] = {k: {"launches": ctx.timing_get(k)[0], "ms": round(ctx.timing_get(k)[1], 4)} for k in slots}
    ctx.timing(False)
    return r


def measure(ctx, kind, scale, ef):
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, 1)
    g = api.Graph.from_coo(ctx, V, src, dst, with_incoming=False)
    del src, dst
    row = {"graph": "%s-%dx%d" % (kind, scale, ef), "V": V, "E": g.E}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.prepare_similarity()
    torch.cuda.synchronize()
    row["prepare_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    print(json.dumps(row), flush=True)

    edges = api.maximal_matching(g, raw=True)[1]["edges"]
    eu, ev = edges[:, 0].contiguous(), edges[:, 1].contiguous()
    del edges
    torch.cuda.empty_cache()
    row["undirected_edges"] = int(eu.numel())
    row["all_edges"] = workload(ctx, lambda: api._sim_pairs(g, eu, ev)[3], PAIR_SLOTS)
    print(json.dumps(row["all_edges"]), flush=True)
    del eu, ev
    torch.cuda.empty_cache()

    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    u = torch.randint(0, V, (RANDOM_PAIRS,), dtype=torch.int32, device=ctx.device, generator=gen)
    v = torch.randint(0, V, (RANDOM_PAIRS,), dtype=torch.int32, device=ctx.device, generator=gen)
    row["random_pairs"] = workload(ctx, lambda: api._sim_pairs(g, u, v)[3], PAIR_SLOTS)
    print(json.dumps(row["random_pairs"]), flush=True)
    del u, v

    deg = api._sim_degree(g)
    queries = torch.nonzero(deg > 0).flatten()[:QUERIES].to(torch.int32)
    row["top10_jaccard"] = workload(ctx, lambda: api.link_prediction(g, k=10, metric="jaccard", vertices=queries, raw=True)[3], TOPK_SLOTS)
    print(json.dumps(row["top10_jaccard"]), flush=True)
    g.close()
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
