#!/usr/bin/env python3
"""What DESIGN section 29 quotes for the neighbour aggregation (GPU box).  On one graph, in the incoming direction: the plan and the transpose build
(median of 3 builds each), then per width F the forward SUM and its backward through the C calls (host clock around a call that ends in a device
synchronise; two warm-up calls, the median of 7, the smallest and the largest stated), the bytes model of the stats, its share of 8 TB/s and of the
copy rate on record (5.15 TB/s, section 9), the event brackets per timing slot from a run of their own, and what a user had at the parent commit, in
the same process on the same GPU: out.index_add_(0, row_of_entry, x[adj]) and torch.sparse.mm on a CSR tensor where this build has it (timed with
torch.cuda.synchronize() around, the same warm-up and repetitions).  Nothing here gates anything.
usage: python3 tests/studies/agg_measure.py OUT.json [kind:scale:edge_factor] [F ...]    (default rmat:20:16 and 16 64 256)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from vectorgraphlibrary_amd import api, lib

SLOTS = ["agg_prepare", "agg_transpose", "agg_short", "agg_wave", "agg_wg", "agg_hubs"]
WARM, REPS, BUILDS = 2, 7, 3
PEAK, COPY = 8.0e12, 5.15e12


def timed(fn, sync):
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(REPS):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def rate(row, stats):
    row["stats"] = stats
    row["model_TBps"] = round(stats["algorithmic_bytes"] / (row["ms_median"] * 1e-3) / 1e12, 3)
    row["of_8TBps"], row["of_copy_rate"] = round(row["model_TBps"] * 1e12 / PEAK, 3), round(row["model_TBps"] * 1e12 / COPY, 3)
    return row


def slots(ctx, fn):
    ctx.timing(True)
    fn()
    out = {k: {"launches": ctx.timing_get(k)[0], "ms": round(ctx.timing_get(k)[1], 4)} for k in SLOTS}
    ctx.timing(False)
    return out


def main():
    args = sys.argv[1:]
    out_path = args.pop(0)
    kind, scale, ef = (args.pop(0) if args and ":" in args[0] else "rmat:20:16").split(":")
    widths = [int(a) for a in args] or [16, 64, 256]
    scale, ef = int(scale), int(ef)
    V = 1 << scale
    ctx = api.Context(0)
    sync = torch.cuda.synchronize
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, 1)
    g = api.Graph.from_coo(ctx, V, src, dst)
    del src, dst
    rowptr, adj = g.in_rowptr, g.in_adj
    report = {"graph": "%s-%dx%d" % (kind, scale, ef), "V": V, "E": g.E, "direction": "in", "widths": {}}
    # the plan and the transpose, built afresh each time (the transpose through a first backward run at F = 1)
    one, gone = torch.ones((V, 1), device=ctx.device), torch.empty((V, 1), device=ctx.device)
    plan_ms, tr_ms = [], []
    for i in range(BUILDS + 1):
        sync()
        t0 = time.perf_counter()
        plan = api.AggregationPlan(ctx, rowptr, adj, V)
        t1 = time.perf_counter()
        plan._backward(one, 0, None, None)
        t2 = time.perf_counter()
        plan._backward(one, 0, None, None)
        t3 = time.perf_counter()
        if i:
            plan_ms.append((t1 - t0) * 1e3)
            tr_ms.append(((t2 - t1) - (t3 - t2)) * 1e3)
        if i < BUILDS:
            plan.close()
    report["plan_ms"] = {"median": round(statistics.median(plan_ms), 3), "all": [round(x, 3) for x in plan_ms]}
    report["transpose_ms"] = {"median": round(statistics.median(tr_ms), 3), "all": [round(x, 3) for x in tr_ms], "note": "first backward run less a later one"}
    report["plan_info"], report["transposed_info"] = plan.info(), plan.last_backward_stats
    print(json.dumps({k: report[k] for k in ("graph", "plan_ms", "transpose_ms", "plan_info")}), flush=True)
    row_of_entry = torch.repeat_interleave(torch.arange(V, device=ctx.device), rowptr[1:] - rowptr[:-1])
    adj64 = adj.long()
    for F in widths:
        x = torch.randn((V, F), device=ctx.device)
        gout = torch.randn((V, F), device=ctx.device)
        r = {}
        r["forward_sum"] = rate(timed(lambda: plan._forward(x, 0, None), sync), plan.last_stats)
        r["forward_sum"]["slots"] = slots(ctx, lambda: plan._forward(x, 0, None))
        r["backward_sum"] = rate(timed(lambda: plan._backward(gout, 0, None, None), sync), plan.last_backward_stats)
        r["backward_sum"]["slots"] = slots(ctx, lambda: plan._backward(gout, 0, None, None))
        want = plan._forward(x, 0, None)[0]

        def index_add():
            return torch.zeros((V, F), device=ctx.device).index_add_(0, row_of_entry, x[adj64])
        try:
            r["torch_index_add"] = timed(index_add, sync)
            r["torch_index_add"]["largest_difference"] = float((index_add() - want).abs().max())
        except RuntimeError as e:
            r["torch_index_add"] = {"error": str(e)[:200]}
        try:
            A = torch.sparse_csr_tensor(rowptr, adj64, torch.ones(g.E, device=ctx.device), size=(V, V))
            r["torch_sparse_mm"] = timed(lambda: torch.sparse.mm(A, x), sync)
            r["torch_sparse_mm"]["largest_difference"] = float((torch.sparse.mm(A, x) - want).abs().max())
            del A
        except (RuntimeError, NotImplementedError) as e:
            r["torch_sparse_mm"] = {"error": str(e)[:200]}
        if "ms_median" in r["torch_index_add"]:
            r["forward_over_index_add"] = round(r["forward_sum"]["ms_median"] / r["torch_index_add"]["ms_median"], 3)
        report["widths"][str(F)] = r
        print("F", F, json.dumps(r), flush=True)
        with open(out_path, "w") as f:
            json.dump(report, f, indent=1)
        del x, gout, want
        torch.cuda.empty_cache()
    plan.close()
    g.close()


if __name__ == "__main__":
    main()
