#!/usr/bin/env python3
"""What DESIGN section 30 quotes for the edge scores, the edge softmax, the differentiable weighted aggregation and graph attention (GPU box), by the
method of agg_measure.py.  On one graph, in the incoming direction, at one width F: each of sddmm, edge_softmax, spmm and graph_attention, forward
(the API call under torch.no_grad) and forward + backward (the call on leaves that require grad, then .backward() of a fixed gradient), with a host
clock around calls that end in a device synchronise; two warm-up calls, the median of 7, the smallest and the largest stated.  The forward C calls
state the bytes model of their stats and its share of the copy rate on record (5.15 TB/s, section 9).  The baseline is the torch formulation in the
same process on the same GPU: (q[row] * k[adj]).sum(-1) for the score, a scatter-max / index_add_ softmax, an index_add_ aggregation, and autograd
through them.  Nothing here gates anything.
usage: python3 tests/studies/edge_measure.py OUT.json [kind:scale:edge_factor] [F]    (default rmat:20:16 and 64)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from vectorgraphlibrary_amd import api

WARM, REPS = 2, 7
PEAK, COPY = 8.0e12, 5.15e12


def timed(fn):
    sync = torch.cuda.synchronize
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
    row["algorithmic_bytes"] = stats["algorithmic_bytes"]
    row["model_TBps"] = round(stats["algorithmic_bytes"] / (row["ms_median"] * 1e-3) / 1e12, 3)
    row["of_copy_rate"] = round(row["model_TBps"] * 1e12 / COPY, 3)
    return row


def both(make, leaves, grad):
    """forward alone, and forward + backward on fresh leaves"""
    def fwd():
        with torch.no_grad():
            return make(*leaves)

    def fwd_bwd():
        ls = [t.detach().requires_grad_(True) for t in leaves]
        make(*ls).backward(grad)
        return [t.grad for t in ls]
    return fwd, fwd_bwd


def main():
    args = sys.argv[1:]
    out_path = args.pop(0)
    kind, scale, ef = (args.pop(0) if args and ":" in args[0] else "rmat:20:16").split(":")
    F = int(args[0]) if args else 64
    scale, ef = int(scale), int(ef)
    V = 1 << scale
    ctx = api.Context(0)
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, 1)
    g = api.Graph.from_coo(ctx, V, src, dst)
    del src, dst
    rowptr, adj = g.in_rowptr, g.in_adj
    E = g.E
    plan = api.AggregationPlan(ctx, rowptr, adj, V)
    row = torch.repeat_interleave(torch.arange(V, device=ctx.device), rowptr[1:] - rowptr[:-1])
    adj64 = adj.long()
    torch.manual_seed(1)
    q, k, v = (torch.randn((V, F), device=ctx.device) * 0.5 for _ in range(3))
    e, w = torch.rand(E, device=ctx.device) * 16 - 8, torch.rand(E, device=ctx.device)
    g_e, g_out = torch.randn(E, device=ctx.device), torch.randn((V, F), device=ctx.device)
    sc = F ** -0.5

    def t_dot(a, b):
        return (a[row] * b[adj64]).sum(-1)

    def t_softmax(x):
        m = torch.full((V,), float("-inf"), device=ctx.device).scatter_reduce(0, row, x.detach(), "amax")
        t = torch.exp(x - m[row])
        return t / torch.zeros(V, device=ctx.device).index_add_(0, row, t)[row]

    def t_spmm(wt, x):
        return torch.zeros((V, F), device=ctx.device).index_add_(0, row, wt[:, None] * x[adj64])

    cases = {
        "sddmm": (lambda a, b: api.sddmm(plan, a, b), t_dot, (q, k), g_e),
        "edge_softmax": (lambda x: api.edge_softmax(plan, x), t_softmax, (e,), g_e),
        "spmm": (lambda wt, x: api.spmm(plan, wt, x), t_spmm, (w, v), g_out),
        "graph_attention": (lambda a, b, c: api.graph_attention(plan, a, b, c), lambda a, b, c: t_spmm(t_softmax(t_dot(a, b) * sc), c), (q, k, v), g_out),
    }
    report = {"graph": "%s-%dx%d" % (kind, scale, ef), "V": V, "E": E, "F": F, "direction": "in", "plan_info": plan.info(), "calls": {}}
    api.sddmm(plan, q.clone().requires_grad_(True), k.clone().requires_grad_(True)).backward(g_e)       # (the transpose is built before anything is timed)
    for name, (ours, theirs, leaves, grad) in cases.items():
        r = {}
        for who, make in (("hip", ours), ("torch", theirs)):
            fwd, fwd_bwd = both(make, leaves, grad)
            try:
                r[who + "_forward"] = timed(fwd)
                if who == "hip" and name != "graph_attention":
                    rate(r[who + "_forward"], plan.last_stats if name == "spmm" else plan.last_edge_stats)
                r[who + "_forward_backward"] = timed(fwd_bwd)
            except RuntimeError as err:
                r[who + "_error"] = str(err)[:200]
            torch.cuda.empty_cache()
        if "hip_error" not in r and "torch_error" not in r:
            a, b = both(ours, leaves, grad), both(theirs, leaves, grad)
            r["largest_forward_difference"] = float((a[0]() - b[0]()).abs().max())
            r["largest_gradient_difference"] = max(float((x - y).abs().max()) for x, y in zip(a[1](), b[1]()))
            r["forward_speedup"] = round(r["torch_forward"]["ms_median"] / r["hip_forward"]["ms_median"], 2)
            r["forward_backward_speedup"] = round(r["torch_forward_backward"]["ms_median"] / r["hip_forward_backward"]["ms_median"], 2)
        report["calls"][name] = r
        print(name, json.dumps(r), flush=True)
        with open(out_path, "w") as f:
            json.dump(report, f, indent=1)
    plan.close()
    g.close()


if __name__ == "__main__":
    main()
