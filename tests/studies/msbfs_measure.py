#!/usr/bin/env python3
"""What DESIGN section 19 quotes for the multi-source BFS (GPU box): one batch of 64 sources against the same 64 sources through vgl_hip_bfs_run_batch,
the per-kernel split, the VGL_MSBFS_PULL_SHARE sweep and the dominant kernel's algorithmic bytes over time.  Every timed figure is the mean of `reps`
calls (40; 10 from scale 22 on) after one warm-up call, host clock around a call that ends in a device synchronise; the per-kernel figures come from a run of their own with
the event brackets on.  The per-source outputs of every schedule are compared with the push-only run's.
usage: python3 tests/studies/msbfs_measure.py OUT.json [kind:scale:edge_factor ...]    (default rmat:20:32 uniform:20:32)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from vectorgraphlibrary_amd import api

SLOTS = ["msbfs_push_short", "msbfs_push_wave", "msbfs_push_wg", "msbfs_pull_short", "msbfs_pull_wave", "msbfs_pull_wg", "msbfs_settle", "msbfs_publish"]
SHARES = ["0.01", "0.02", "0.05", "0.1", "0.2", "push"]
HBM_PEAK = 8.0e12
reps = 40


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def setting(share):
    os.environ.pop("VGL_MSBFS_MODE", None)
    os.environ.pop("VGL_MSBFS_PULL_SHARE", None)
    if share == "push":
        os.environ["VGL_MSBFS_MODE"] = "push"
    elif share is not None:
        os.environ["VGL_MSBFS_PULL_SHARE"] = share


def measure(ctx, kind, scale, ef):
    global reps
    reps = 40 if scale < 22 else 10
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, 1)
    g = api.Graph.from_coo(ctx, V, src, dst)
    del src, dst
    deg = g.out_rowptr[1:] - g.out_rowptr[:-1]
    sources = torch.nonzero(deg > 0).flatten()[:64].tolist()              # the app's choice
    g.prepare_msbfs("out")
    row = {"graph": "%s-%dx%d" % (kind, scale, ef), "V": V, "E": g.E, "sources": len(sources)}
    setting("push")
    want = api.multi_source_bfs(g, sources, raw=True)[0]
    row["sweep_ms"] = {}
    for share in SHARES:
        setting(share)
        ms, (got, st) = timed(lambda: api.multi_source_bfs(g, sources, raw=True))
        assert all(torch.equal(got[k], want[k]) for k in want), share
        row["sweep_ms"][share] = round(ms, 4)
        row.setdefault("stats", {})[share] = st
    setting(None)
    ms, (_, st) = timed(lambda: api.multi_source_bfs(g, sources, raw=True))
    row["msbfs_batch_ms"] = round(ms, 4)
    ms, _ = timed(lambda: api.bfs_batch(g, sources))
    row["bfs_run_batch_64_ms"] = round(ms, 4)
    row["single_over_batch"] = round(row["bfs_run_batch_64_ms"] / row["msbfs_batch_ms"], 3)
    ctx.timing(True)
    _, st = api.multi_source_bfs(g, sources, raw=True)
    torch.cuda.synchronize()
    row["kernels"] = {k: {"launches": ctx.timing_get(k)[0], "ms": round(ctx.timing_get(k)[1], 4)} for k in SLOTS}
    ctx.timing(False)
    # the bytes model of the pull kernels (12 per entry examined, 12 V per level) and of the push kernels (12 per entry, 28 per frontier vertex left out)
    pull_ms = sum(row["kernels"][k]["ms"] for k in SLOTS[3:6])
    push_ms = sum(row["kernels"][k]["ms"] for k in SLOTS[:3])
    pull_bytes = 12 * st["edges_pull"] + 12 * V * st["levels_pull"]
    push_bytes = 12 * st["edges_push"]
    row["pull"] = {"ms": round(pull_ms, 4), "bytes": pull_bytes, "share_of_hbm_peak": round(pull_bytes / max(pull_ms, 1e-9) / 1e-3 / HBM_PEAK, 4)}
    row["push"] = {"ms": round(push_ms, 4), "bytes": push_bytes, "share_of_hbm_peak": round(push_bytes / max(push_ms, 1e-9) / 1e-3 / HBM_PEAK, 4)}
    row["stats_default"] = st
    g.close()
    return row


def main():
    out = sys.argv[1]
    graphs = sys.argv[2:] or ["rmat:20:32", "uniform:20:32"]
    ctx = api.Context(0)
    rows = []
    for spec in graphs:
        kind, scale, ef = spec.split(":")
        rows.append(measure(ctx, kind, int(scale), int(ef)))
        print(json.dumps(rows[-1]), flush=True)
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
