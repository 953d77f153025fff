#!/usr/bin/env python3
"""What DESIGN section 22 quotes for the maximal independent set and the maximal matching (GPU box): the prepare times, the time of a run (the median
of 5 calls after one warm-up call, host clock around a call that ends in a device synchronise), the per-slot split from a run of its own with the
event brackets on, rounds / live_total / entries_walked, and the bytes model of include/vgl_hip.h over the run time as a share of the HBM peak.  The
yardstick is not this code: it is the sequential host greedy that `apps/bin/mis_hip [-matching] -check` runs and times on the same generated graph
(-no-app skips it).
usage: python3 tests/studies/mis_measure.py OUT.json [-no-app] [kind:scale:edge_factor ...]    (default rmat:20:16)"""
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

SLOTS = {"mis": ["mis_init", "mis_short", "mis_wave", "mis_wg", "mis_publish", "mis_finish"],
         "matching": ["mm_init", "mm_best_short", "mm_best_wave", "mm_best_wg", "mm_match", "mm_publish"]}
HBM_PEAK = 8.0e12
REPS = 5
SEED = 1                                                                      # the app's default seed: the same keys as its runs


def timed(ctx, call):
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        st = call()[1]
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times, st


def measure(ctx, kind, scale, ef, with_app):
    V = 1 << scale
    src, dst = (ctx.gen_rmat if kind == "rmat" else ctx.gen_uniform)(scale, ef, 1)
    g = api.Graph.from_coo(ctx, V, src, dst, with_incoming=False)
    del src, dst
    row = {"graph": "%s-%dx%d" % (kind, scale, ef), "V": V, "E": g.E}
    for what, prepare, call in (("mis", g.prepare_mis, lambda: api.maximal_independent_set(g, seed=SEED, rounds=True, raw=True)),
                                ("matching", g.prepare_matching, lambda: api.maximal_matching(g, seed=SEED, raw=True))):
        r = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prepare()
        torch.cuda.synchronize()
        r["prepare_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        times, st = timed(ctx, call)
        r["run_ms"] = [round(t, 3) for t in times]
        r["run_ms_median"] = round(statistics.median(times), 3)
        r["stats"] = {k: v for k, v in st.items() if not torch.is_tensor(v)}
        r["share_of_hbm_peak"] = round(st["algorithmic_bytes"] / (r["run_ms_median"] * 1e-3) / HBM_PEAK, 4)
        ctx.timing(True)
        call()
        torch.cuda.synchronize()
        r["kernels"] = {k: {"launches": ctx.timing_get(k)[0], "ms": round(ctx.timing_get(k)[1], 4)} for k in SLOTS[what]}
        ctx.timing(False)
        if with_app:
            cmd = [os.path.join(ROOT, "apps", "bin", "mis_hip"), "-gen", "-type", kind, "-s", str(scale), "-e", str(ef), "-fused", "-check"] + (["-matching"] if what == "matching" else [])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            m = re.search(r"host greedy[^:]*: ([0-9.e+-]+) ms", out.stdout)
            r["host_greedy_ms"] = float(m.group(1)) if m else None
            r["app_check"] = "error count: 0" in out.stdout and out.returncode == 0
            r["app_returncode"] = out.returncode
            r["app_lines"] = [l for l in out.stdout.splitlines() if l.startswith("MIS") or l.startswith("MATCHING")]
            if not r["app_check"]:                                            # keep what the app said
                r["app_tail"] = (out.stdout + out.stderr)[-2000:]
        row[what] = r
    g.close()
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
