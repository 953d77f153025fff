#!/usr/bin/env python3
"""What DESIGN section 20 quotes for biconnectivity (GPU box): the prepare time, the time of a full run (all five outputs; the median of 5 calls after
one warm-up call, host clock around a call that ends in a device synchronise), the per-slot split from a run of its own with the event brackets on,
the depth, and the dominant kernel family's share of the HBM peak on its part of the bytes model of include/vgl_hip.h.  The yardstick is not this
code: it is the sequential host Hopcroft-Tarjan that `apps/bin/bicc_hip -check` runs and times on the same generated graph (-no-app skips it).
usage: python3 tests/studies/bicc_measure.py OUT.json [-no-app] [kind:scale:edge_factor ...]    (default rmat:20:16)"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from vectorgraphlibrary_amd import api

SLOTS = ["bicc_classify", "bicc_roots", "bicc_seed", "bicc_bfs_short", "bicc_bfs_wave", "bicc_bfs_wg", "bicc_publish", "bicc_size", "bicc_pre", "bicc_local_short",
         "bicc_local_wave", "bicc_local_wg", "bicc_lowhigh", "bicc_reset", "bicc_edge", "bicc_flatten", "bicc_block", "bicc_art_short", "bicc_art_wave", "bicc_art_wg", "bicc_twoecc"]
HBM_PEAK = 8.0e12
REPS = 5


def family_bytes(V, E, nnz):
    """the parts of the bytes model per kernel family (the terms of include/vgl_hip.h, by the pass that moves them)"""
    return {"roots": 8 * E, "bfs": 24 * V + 8 * nnz, "pre": 16 * V, "local": 28 * V + 8 * nnz, "reset": 16 * V, "edge": 17 * E, "flatten": 8 * V, "block": 4 * V + 20 * E, "art": 9 * V + 8 * nnz,
            "twoecc": 8 * V}


def measure(ctx, kind, scale, ef, with_app):
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, 1)
    g = api.Graph.from_coo(ctx, V, src, dst)
    del src, dst
    row = {"graph": "%s-%dx%d" % (kind, scale, ef), "V": V, "E": g.E}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    row["undirected_edges"] = g.prepare_bicc()
    torch.cuda.synchronize()
    row["prepare_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    api.biconnected_components(g, raw=True)
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        _, st = api.biconnected_components(g, raw=True)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    row["run_ms"] = [round(t, 3) for t in times]
    row["run_ms_median"] = round(statistics.median(times), 3)
    row["stats"] = {k: v for k, v in st.items() if not torch.is_tensor(v)}
    api.bridges(g, raw=True)                                                  # measured like the full run: a warm-up call, then the median of 5
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        api.bridges(g, raw=True)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    row["bridges_only_ms"] = [round(t, 3) for t in times]
    row["bridges_only_ms_median"] = round(statistics.median(times), 3)
    ctx.timing(True)
    api.biconnected_components(g, raw=True)
    torch.cuda.synchronize()
    row["kernels"] = {k: {"launches": ctx.timing_get(k)[0], "ms": round(ctx.timing_get(k)[1], 4)} for k in SLOTS}
    ctx.timing(False)
    E = row["undirected_edges"]
    fam = {}
    for name, b in family_bytes(V, E, 2 * E).items():
        ms = sum(v["ms"] for k, v in row["kernels"].items() if k == "bicc_" + name or k.startswith("bicc_" + name + "_"))
        fam[name] = {"ms": round(ms, 4), "bytes": b, "share_of_hbm_peak": round(b / max(ms, 1e-9) / 1e-3 / HBM_PEAK, 4)}
    row["families"] = fam
    row["dominant"] = max(fam, key=lambda k: fam[k]["ms"])
    g.close()
    if with_app:
        cmd = [os.path.join(ROOT, "apps", "bin", "bicc_hip"), "-gen", "-type", kind, "-s", str(scale), "-e", str(ef), "-fused", "-check"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        m = re.search(r"BICC host Hopcroft-Tarjan[^:]*: ([0-9.e+-]+) ms", out.stdout)
        row["host_hopcroft_tarjan_ms"] = float(m.group(1)) if m else None
        row["app_check"] = "error count: 0" in out.stdout and out.returncode == 0
        row["app_returncode"] = out.returncode
        row["app_lines"] = [l for l in out.stdout.splitlines() if l.startswith("BICC")]
        if not row["app_check"]:                                              # keep what the app said
            row["app_tail"] = (out.stdout + out.stderr)[-2000:]
    return row


def main():
    args = sys.argv[1:]
    out = args.pop(0)
    with_app = "-no-app" not in args
    graphs = [a for a in args if a != "-no-app"] or ["rmat:20:16"]
    ctx = api.Context(0)
    rows = []
    for spec in graphs:
        kind, scale, ef = spec.split(":")
        rows.append(measure(ctx, kind, int(scale), int(ef), with_app))
        print(json.dumps(rows[-1]), flush=True)
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
