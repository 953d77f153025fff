#!/usr/bin/env python3
"""What DESIGN section 31 quotes for heads (GPU box), by the method of edge_measure.py.  On one graph, in the incoming direction, for every (F, H) of
the list: each of sddmm, edge_softmax, spmm and graph_attention with H heads in one call, forward (under torch.no_grad) and forward + backward (fresh
leaves that require grad, .backward() of a fixed gradient, the transpose built beforehand), with a host clock around calls that end in a device
synchronise; two warm-up calls, the median of 7, the smallest and the largest stated.  Two baselines in the same process: what a user does without
the heads calls -- H single-head calls on column slices (H separate E-vectors between them) and one torch.stack / torch.cat -- ALTERNATED with the
heads call, one after the other inside every repetition; and the torch formulation of edge_measure.py reshaped to heads.  With H = 1 the slice loop
is the single-head call itself, so that row states what the new entry points cost beside the existing ones.  The forward C calls state the bytes
model of their stats and its share of the copy rate on record (5.15 TB/s, section 9).  Nothing here gates anything.
usage: python3 tests/studies/heads_measure.py OUT.json [kind:scale:edge_factor] [F:H ...] [notorch]    (default rmat:20:16 and 64:1 64:4 64:8 128:8)"""
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
    shapes = [tuple(int(x) for x in a.split(":")) for a in args if a.count(":") == 1] or [(64, 1), (64, 4), (64, 8), (128, 8)]
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
    report = {"graph": "%s-%dx%d" % (kind, scale, ef), "V": V, "E": E, "direction": "in", "plan_info": plan.info(), "shapes": {}}
    plan._backward(torch.zeros((V, 4), device=ctx.device), 0, None, None)                       # (the transpose is built before anything is timed)
    for F, H in shapes:
        D = F // H
        cols = [slice(h * D, (h + 1) * D) for h in range(H)]
        torch.manual_seed(1)
        q, k, v = (torch.randn((V, F), device=ctx.device) * 0.5 for _ in range(3))
        e, w = torch.rand((E, H), device=ctx.device) * 16 - 8, torch.rand((E, H), device=ctx.device)
        e_h, w_h = [e[:, h].contiguous() for h in range(H)], [w[:, h].contiguous() for h in range(H)]
        g_e, g_out = torch.randn((E, H), device=ctx.device), torch.randn((V, F), device=ctx.device)
        sc = D ** -0.5

        def t_dot(a, b):
            return (a[row].view(E, H, D) * b[adj64].view(E, H, D)).sum(-1)

        def t_softmax(x):
            m = torch.full((V, H), float("-inf"), device=ctx.device).scatter_reduce(0, row[:, None].expand(E, H), x.detach(), "amax")
            t = torch.exp(x - m[row])
            return t / torch.zeros((V, H), device=ctx.device).index_add_(0, row, t)[row]

        def t_spmm(wt, x):
            return torch.zeros((V, H, D), device=ctx.device).index_add_(0, row, wt[:, :, None] * x[adj64].view(E, H, D)).view(V, F)

        if H == 1:          # the slice loop of one head is the single-head call
            s_dot = lambda a, b: api.sddmm(plan, a, b)[:, None]  # noqa: E731
            s_softmax = lambda x: api.edge_softmax(plan, x)[:, None]  # noqa: E731
            s_spmm = lambda wt, x: api.spmm(plan, wt, x)  # noqa: E731
            s_attention = lambda a, b, c: api.graph_attention(plan, a, b, c)  # noqa: E731
        else:
            s_dot = lambda a, b: torch.stack([api.sddmm(plan, a[:, c], b[:, c]) for c in cols], 1)  # noqa: E731
            s_softmax = lambda *xs: torch.stack([api.edge_softmax(plan, x) for x in xs], 1)  # noqa: E731
            s_spmm = lambda *t: torch.cat([api.spmm(plan, wt, t[-1][:, c]) for wt, c in zip(t[:-1], cols)], 1)  # noqa: E731
            s_attention = lambda a, b, c: torch.cat([api.graph_attention(plan, a[:, s], b[:, s], c[:, s], scale=sc) for s in cols], 1)  # noqa: E731
        # name: (the heads call, its leaves, the slice loop, its leaves, the torch form, the gradient)
        cases = {
            "sddmm": (lambda a, b: api.sddmm(plan, a, b, heads=H), (q, k), s_dot, (q, k), t_dot, g_e),
            # (api.edge_softmax refuses E x 1; graph_attention(heads=1) reaches the heads call the same way)
            "edge_softmax": (lambda x: api._edge_softmax_any(plan, x), (e,), s_softmax, tuple(e_h), t_softmax, g_e),
            "spmm": (lambda wt, x: api.spmm(plan, wt, x), (w, v), s_spmm, tuple(w_h) + (v,), t_spmm, g_out),
            "graph_attention": (lambda a, b, c: api.graph_attention(plan, a, b, c, heads=H), (q, k, v), s_attention, (q, k, v),
                                lambda a, b, c: t_spmm(t_softmax(t_dot(a, b) * sc), c), g_out),
        }
        shape = report["shapes"].setdefault("F=%d,H=%d" % (F, H), {})
        for name, (ours, leaves, theirs, their_leaves, torch_form, grad) in cases.items():
            r = {}
            a, b = both(ours, leaves, grad), both(theirs, their_leaves, grad)
            r["heads_forward"], r["slices_forward"] = timed(a[0], b[0])
            if name != "graph_attention":
                a[0]()
                rate(r["heads_forward"], plan.last_stats if name == "spmm" else plan.last_edge_stats)
            r["heads_forward_backward"], r["slices_forward_backward"] = timed(a[1], b[1])
            r["same_bits_as_slices"] = bool(torch.equal(a[0]().view(torch.int32), b[0]().contiguous().view(torch.int32)))
            r["forward_over_slices"] = round(r["slices_forward"]["ms_median"] / r["heads_forward"]["ms_median"], 2)
            r["forward_backward_over_slices"] = round(r["slices_forward_backward"]["ms_median"] / r["heads_forward_backward"]["ms_median"], 2)
            if with_torch:
                try:
                    t = both(torch_form, leaves, grad)
                    (r["torch_forward"],), (r["torch_forward_backward"],) = timed(t[0]), timed(t[1])
                    r["largest_forward_difference"] = float((a[0]() - t[0]()).abs().max())
                    r["forward_over_torch"] = round(r["torch_forward"]["ms_median"] / r["heads_forward"]["ms_median"], 2)
                    r["forward_backward_over_torch"] = round(r["torch_forward_backward"]["ms_median"] / r["heads_forward_backward"]["ms_median"], 2)
                except RuntimeError as err:
                    r["torch_error"] = str(err)[:200]
                torch.cuda.empty_cache()
            shape[name] = r
            print("F=%d H=%d" % (F, H), name, json.dumps(r), flush=True)
            with open(out_path, "w") as f:
                json.dump(report, f, indent=1)
    plan.close()
    g.close()


if __name__ == "__main__":
    main()
