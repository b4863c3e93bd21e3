"""The figures of profiles/essential_graph.md for Optimizer::OptimizeEssentialGraph (cms_essential_graph_optimize): one synchronous call host to host (a
host clock around a call that ends in a stream synchronise; the job array is laid out outside the clock) for 1 and 8 jobs at N = 120 and N = 1031
(1030 free vertices), against hm_essential_graph_optimize_host on the same records on one CPU thread of the same machine.  Three warm-up calls per
shape; the window repeats the call for at least 1.5 s and five times.  One JSON row per shape on stdout.  Needs a device.

    python tools/prof_ess_graph.py [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import ess_graph_cases as gc
import ess_graph_hostlib as hl
from cubemapslam_amd import api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = api.Context(synth.camera("lafida", 150), nfeatures=500, max_batch=1, device=0)
opt = api.EssentialGraphOptimizer(8, 8 * 1031, 8 * 3200, 8 * 11000, device=0)
rows = []
for N in (120, 1031):
    graphs = [gc.graph(200 + j, N, j % 2) for j in range(8)]
    for njobs in (1, 8):
        make = lambda: [api.ess_graph_job_state(g) for g in graphs[:njobs]]
        st = make()
        blocks = [hl.envelope(s["N"], s["fixed"], s["edges"])[1] for s in st]
        for _ in range(3):
            res = opt.run(ctx, make())
        times = []
        t_end = time.perf_counter() + 1.5
        while time.perf_counter() < t_end or len(times) < 5:
            arr = api.ess_graph_jobs(st)
            t0 = time.perf_counter(); opt.optimize(ctx, arr, njobs); times.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); rc, want = hl.optimize_host(make()); t_host = time.perf_counter() - t0
        same = api.ess_graph_first_difference(want, res) is None
        rows.append(dict(N=N, njobs=njobs, edges=[s["E"] for s in st], envelope_blocks=blocks, trials=[r["trials_run"] for r in res], iterations=[r["iterations_run"] for r in res],
                         device_ms_median=1e3 * float(np.median(times)), device_ms_min=1e3 * min(times), device_ms_max=1e3 * max(times), calls=len(times),
                         host_core_ms=1e3 * t_host, equal_bits=bool(same)))
        print(json.dumps(rows[-1]), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
opt.close(); ctx.close()
