#!/usr/bin/env python3
"""What DESIGN section 32 quotes for the additive score of GAT (GPU box), by the method of heads_measure.py.  On one graph, in the incoming
direction, for every H of the list (F = 64 for the whole layer): the score u_add_v, the two entry sums (the gated ones that are its gradients), and
gat_attention forward (under torch.no_grad) and forward + backward (fresh leaves that require grad, .backward() of a fixed gradient, the transpose
built beforehand), with a host clock around calls that end in a device synchronise; two warm-up calls, the median of 7, the smallest and the
largest stated.  The baseline in the same process, ALTERNATED with our call inside every repetition, is the torch formulation a user writes without
these calls: row-index gathers s[row] + t[adj], leaky_relu, a scatter-max softmax, index_add_ for the sums (floating-point atomics: its bits change
from run to run).  The C calls state the bytes model of their stats and its share of the copy rate on record (5.15 TB/s, section 9).  Nothing
here gates anything.
usage: python3 tests/studies/gat_measure.py OUT.json [kind:scale:edge_factor] [H ...] [notorch]    (default rmat:20:16 and 1 4 8)"""
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
COPY = 5.15e12
F = 64
SLOPE = 0.2


def summary(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def timed(*fns):
    """the functions one after the other inside every repetition: one summary each"""
    sync = torch.cuda.synchronize
    for _ in range(WARM):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(REPS):
        for fn, to in zip(fns, ms):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            to.append((time.perf_counter() - t0) * 1e3)
    return [summary(m) for m in ms]


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
    kind, scale, ef = (args.pop(0) if args and args[0].count(":") == 2 else "rmat:20:16").split(":")
    with_torch = "notorch" not in args
    heads = [int(a) for a in args if a.isdigit()] or [1, 4, 8]
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
    report = {"graph": "%s-%dx%d" % (kind, scale, ef), "V": V, "E": E, "F": F, "direction": "in", "plan_info": plan.info(), "heads": {}}
    plan._backward(torch.zeros((V, 4), device=ctx.device), 0, None, None)                       # (the transpose is built before anything is timed)
    for H in heads:
        D = F // H
        torch.manual_seed(1)
        s, t, v = torch.randn((V, H), device=ctx.device), torch.randn((V, H), device=ctx.device), torch.randn((V, F), device=ctx.device) * 0.5
        g_e, g_out = torch.randn((E, H), device=ctx.device), torch.randn((V, F), device=ctx.device)
        e = plan._edge_add(s, t, H, SLOPE)

        def t_score(a, b):
            return torch.nn.functional.leaky_relu(a[row] + b[adj64], SLOPE)

        def t_softmax(x):
            m = torch.full((V, H), float("-inf"), device=ctx.device).scatter_reduce(0, row[:, None].expand(E, H), x.detach(), "amax")
            p = torch.exp(x - m[row])
            return p / torch.zeros((V, H), device=ctx.device).index_add_(0, row, p)[row]

        def t_spmm(wt, x):
            return torch.zeros((V, H, D), device=ctx.device).index_add_(0, row, wt[:, :, None] * x[adj64].view(E, H, D)).view(V, F)

        def t_sum(index):
            return lambda: torch.zeros((V, H), device=ctx.device).index_add_(0, index, torch.where(e > 0, g_e, SLOPE * g_e))

        r = report["heads"].setdefault("H=%d" % H, {})
        # the score: forward, and forward + backward (the two gated sums)
        ours, theirs = both(lambda a, b: api.u_add_v(plan, a, b, SLOPE), (s, t), g_e), both(t_score, (s, t), g_e)
        c = {}
        if with_torch:
            c["forward"], c["torch_forward"] = timed(ours[0], theirs[0])
            c["forward_backward"], c["torch_forward_backward"] = timed(ours[1], theirs[1])
            c["same_bits_as_torch"] = bool(torch.equal(ours[0]().view(torch.int32), theirs[0]().view(torch.int32)))
            c["forward_over_torch"] = round(c["torch_forward"]["ms_median"] / c["forward"]["ms_median"], 2)
            c["forward_backward_over_torch"] = round(c["torch_forward_backward"]["ms_median"] / c["forward_backward"]["ms_median"], 2)
        else:
            (c["forward"],), (c["forward_backward"],) = timed(ours[0]), timed(ours[1])
        ours[0]()
        rate(c["forward"], plan.last_edge_stats)
        r["u_add_v"] = c
        print("H=%d" % H, "u_add_v", json.dumps(c), flush=True)
        # the two gated sums on their own: the C calls
        for name, transposed, index in (("edge_sum_gated", False, row), ("edge_sum_gated_transposed", True, adj64)):
            fn = lambda: plan._edge_sum(g_e, e, SLOPE, transposed)  # noqa: E731
            c = {}
            if with_torch:
                c["ours"], c["torch"] = timed(fn, t_sum(index))
                c["over_torch"] = round(c["torch"]["ms_median"] / c["ours"]["ms_median"], 2)
                c["largest_difference"] = float((fn() - t_sum(index)()).abs().max())
            else:
                (c["ours"],) = timed(fn)
            fn()
            rate(c["ours"], plan.last_edge_stats)
            r[name] = c
            print("H=%d" % H, name, json.dumps(c), flush=True)
        # the whole layer at F = 64
        ours = both(lambda a, b, x: api.gat_attention(plan, a, b, x, SLOPE), (s, t, v), g_out)
        c = {}
        if with_torch:
            try:
                theirs = both(lambda a, b, x: t_spmm(t_softmax(t_score(a, b)), x), (s, t, v), g_out)
                c["forward"], c["torch_forward"] = timed(ours[0], theirs[0])
                c["forward_backward"], c["torch_forward_backward"] = timed(ours[1], theirs[1])
                c["largest_forward_difference"] = float((ours[0]() - theirs[0]()).abs().max())
                c["forward_over_torch"] = round(c["torch_forward"]["ms_median"] / c["forward"]["ms_median"], 2)
                c["forward_backward_over_torch"] = round(c["torch_forward_backward"]["ms_median"] / c["forward_backward"]["ms_median"], 2)
            except RuntimeError as err:
                c["torch_error"] = str(err)[:200]
            torch.cuda.empty_cache()
        if "forward" not in c:
            (c["forward"],), (c["forward_backward"],) = timed(ours[0]), timed(ours[1])
        # the bytes model of the layer's three forward calls
        with torch.no_grad():
            w = api._edge_softmax_any(plan, api.u_add_v(plan, s, t, SLOPE))
            total = plan.last_edge_stats["algorithmic_bytes"]
            api.u_add_v(plan, s, t, SLOPE)
            total += plan.last_edge_stats["algorithmic_bytes"]
            api.spmm(plan, w, v)
            total += plan.last_stats["algorithmic_bytes"]
        rate(c["forward"], {"algorithmic_bytes": total})
        r["gat_attention"] = c
        print("H=%d" % H, "gat_attention", json.dumps(c), flush=True)
        with open(out_path, "w") as f:
            json.dump(report, f, indent=1)
    plan.close()
    g.close()


if __name__ == "__main__":
    main()
