"""Time of cms_sim3_iterate on the device against the host loop it is held to (hm_sim3_iterate_host, one thread), at the shapes of
LoopClosing::ComputeSim3.  min_inliers = N - 1, so no hypothesis is accepted and every call evaluates all of its hypotheses: the work is fixed.

  pass      8 candidates x iterate(5), N = 150            (one pass of the `for` at LoopClosing.cpp:287)
  find      8 candidates x 300 hypotheses, N = 150        (every candidate run to exhaustion in one call)
  many      64 candidates x 300 hypotheses, N = 300       (a host that serves several maps)

Host-to-host time of the synchronous call (one block up, two launches, one block back, one wait): medians over --reps calls after a warm-up, p10 / p90
as the spread.  The kernels' own times come from a run of this script under `rocprofv3 --kernel-trace --stats`.

    python tools/prof_sim3.py [--reps 50]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cubemapslam_amd import api, synth  # noqa: E402
import sim3_cases as sc  # noqa: E402
import sim3_hostlib as hl  # noqa: E402

SHAPES = (("pass", 8, 150, 5), ("find", 8, 150, 300), ("many", 64, 300, 300))


def median_of(fn, reset, reps, warm=3):
    t = []
    for i in range(warm + reps):
        reset()
        t0 = time.perf_counter()
        fn()
        if i >= warm:
            t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    ctx = api.Context(synth.camera("lafida", sc.F), nfeatures=500, max_batch=1, device=0)
    print("| shape | jobs | N | hypotheses per call | device call, ms (p10 - p90) | host loop, ms (p10 - p90) |")
    print("|---|---|---|---|---|---|")
    for name, jobs, N, n_it in SHAPES:
        states = [api.sim3_job_state(sc.problem(700 + j, N=N, outliers=0.4, min_inliers=N - 1, max_its=300), n_it, sc.draws(800 + j, N, 300)) for j in range(jobs)]
        arr = api.sim3_jobs(states)
        solver = api.Sim3Solver(jobs, jobs * N, jobs * 300)

        def reset():
            for q, s in zip(arr, states):
                q.iterations = 0; q.best_inliers = 0
                s["best_mask"][:] = 0
        dev = median_of(lambda: solver.iterate(ctx, arr), reset, a.reps)
        assert all(q.iterations_run == n_it and q.status == 0 for q in arr)
        host = median_of(lambda: hl.H().hm_sim3_iterate_host(sc.F, jobs, arr), reset, max(3, a.reps // 10), warm=1)
        print("| %s | %d | %d | %d | %.3f (%.3f - %.3f) | %.2f (%.2f - %.2f) |" % ((name, jobs, N, jobs * n_it) + dev + host))
        solver.close()
    ctx.close()


if __name__ == "__main__":
    main()
