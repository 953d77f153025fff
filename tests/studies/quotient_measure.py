#!/usr/bin/env python3
"""What DESIGN section 25 quotes for the quotient graph (GPU box).  Per graph, three labelings: hashed labels with K = V / 64, the labels of
label_propagation (5 iterations) and the labels of strongly_connected_components; and one more run of the hashed labels with every row forced into
the sorted class (VGL_QUOT_SHORT = VGL_QUOT_WAVE = VGL_QUOT_TABLE = 0), which shows what the LDS classes buy over the plain sort.  For each: the plan
and the fills (both directions) timed apart, the median of 5 after one warm-up, host clock around calls that end in a device synchronise; the labels
are prepared outside; the event brackets per timing slot from a run of their own.  The one comparison claimed is the sequential host restatement of
apps/bin/quotient_hip -check, which the app prints itself.  Nothing here gates anything: nobody had measured this path.
usage: python3 tests/studies/quotient_measure.py OUT.json [kind:scale:edge_factor ...]    (default rmat:20:16)"""
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

CLASSES = ("short", "wave", "table", "sorted")
SLOTS = ["quot_check", "quot_vertex", "quot_member_off", "quot_classify", "quot_lists"] + ["quot_count_" + k for k in CLASSES] + ["quot_scan", "quot_publish"] + \
        ["quot_fill_" + k for k in CLASSES]
SWITCHES = ("VGL_QUOT_SHORT", "VGL_QUOT_WAVE", "VGL_QUOT_TABLE")
REPS = 5


def fmix32(h):
    h = h & 0xFFFFFFFF
    h = h ^ (h >> 16)
    h = (h * 0x85ebca6b) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    h = (h * 0xc2b2ae35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def plan_and_fill(ctx, g, lab):
    """one plan and the fills of both directions through the C calls; returns (plan ms, fill ms, stats)"""
    ptr = lambda t: C.c_void_p(t.data_ptr())
    plan = C.c_void_p()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lib.check(ctx.L.vgl_hip_quotient_plan_create(ctx.h, g.h, ptr(lab), 0, C.byref(plan)))
    t1 = time.perf_counter()
    try:
        vc, eo, ei, st = C.c_int32(), C.c_int64(), C.c_int64(), lib.QuotientStats()
        lib.check(ctx.L.vgl_hip_quotient_plan_info(plan, C.byref(vc), C.byref(eo), C.byref(ei), C.byref(st)))
        bufs = [(ctx.empty(vc.value + 1, torch.int64), ctx.empty(max(e.value, 1), torch.int32), ctx.empty(max(e.value, 1), torch.int64)) for e in (eo, ei)]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for d, (rp, ad, cnt) in enumerate(bufs):
            lib.check(ctx.L.vgl_hip_quotient_plan_fill(ctx.h, plan, d, None, ptr(rp), ptr(ad), ptr(cnt)))
        ctx.sync()
        t3 = time.perf_counter()
    finally:
        ctx.L.vgl_hip_quotient_plan_destroy(ctx.h, plan)
    return (t1 - t0) * 1e3, (t3 - t2) * 1e3, api._stats(st)


def workload(ctx, g, lab):
    plan_and_fill(ctx, g, lab)
    runs = [plan_and_fill(ctx, g, lab) for _ in range(REPS)]
    r = {"plan_ms": [round(x[0], 3) for x in runs], "fill_ms": [round(x[1], 3) for x in runs], "stats": runs[0][2]}
    r["plan_ms_median"], r["fill_ms_median"] = round(statistics.median(r["plan_ms"]), 3), round(statistics.median(r["fill_ms"]), 3)
    ctx.timing(True)
    plan_and_fill(ctx, g, lab)
    r["kernels"] = {k: {"launches": ctx.timing_get(k)[0], "ms": round(ctx.timing_get(k)[1], 4)} for k in SLOTS}
    ctx.timing(False)
    total = r["plan_ms_median"] + r["fill_ms_median"]
    r["model_GBps"] = round(r["stats"]["algorithmic_bytes"] / (total * 1e-3) / 1e9, 2)
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
    ids = torch.arange(V, dtype=torch.int64, device=ctx.device)
    hashed = (fmix32(ids ^ 1) % max(V // 64, 1)).to(torch.int32)
    labelings = {"hashed_V_over_64": hashed,
                 "label_propagation_5": api.label_propagation(g, max_iterations=5, raw=True)[0].contiguous(),
                 "scc": api.strongly_connected_components(g, raw=True)[0].contiguous()}
    for name, lab in labelings.items():
        row[name] = workload(ctx, g, lab)
        print(name, json.dumps(row[name]), flush=True)
    for k in SWITCHES:
        os.environ[k] = "0"
    row["hashed_V_over_64_all_sorted"] = workload(ctx, g, hashed)
    for k in SWITCHES:
        del os.environ[k]
    print("all sorted", json.dumps(row["hashed_V_over_64_all_sorted"]), flush=True)
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
