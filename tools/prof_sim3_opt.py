"""The figures of profiles/sim3_opt_parity.md for Optimizer::OptimizeSim3 (cms_sim3_optimize):

  CPU part (no GPU needed; the same functions tests/test_sim3_opt_cpu.py asserts on): the distance of the core's exp / sin / cos from libm's in ulps,
  the share of non-zero entries of the as-written Jacobian on the numpy restatement, the analytic Jacobian against central differences, and the
  recovery runs of both modes.
  GPU part: host-to-host time of one synchronous cms_sim3_optimize call (staging, copy up, the launch, copy back, synchronisation; the job array is
  laid out outside the clock) for 1, 8 and 32 jobs of N = 150, outlier share 0.3, both modes, against hm_sim3_optimize_host on the same records on
  the same machine's CPU (one thread); warmed up, median of --reps calls.  Skipped with --cpu-only or when no device is visible.

    python tools/prof_sim3_opt.py [--reps 50] [--cpu-only] [--out profiles/sim3_opt_parity.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import npref_sim3_opt as ref  # noqa: E402
import sim3_opt_cases as sc  # noqa: E402
import sim3_opt_hostlib as hl  # noqa: E402
import test_sim3_opt_cpu as T  # noqa: E402
from cubemapslam_amd import api, synth  # noqa: E402

F = sc.F


def cpu_part():
    out = ["## Measured on the CPU (the functions of tests/test_sim3_opt_cpu.py)", ""]
    d = T.det_libm_distances()
    out.append("- `cms_det_exp` / `cms_det_sincos` against libm over |theta| <= pi, |sigma| <= 1 and the 1e-9 neighbourhood (46 000 arguments): "
               "max %d ulp (exp), %d ulp (sin), %d ulp (cos where |cos| >= 1e-3).  Not a bar: the core is the definition of record." % (d["exp"], d["sin"], d["cos"]))
    c = sc.case(11, N=300, outliers=0.2, fix_scale=0)
    share, med_nz, med_true = T.as_written_nonzero_share(c)
    out.append("- As-written (numeric, delta = 1e-9) Jacobian on the numpy restatement, 300 pairs on five faces, F = %d: %.2f %% of the entries non-zero, "
               "median magnitude of those %.3g, median true magnitude %.3g." % (F, 100 * share, med_nz, med_true))
    S = T.start_of(c); P = ref.make_pairs(F, c)
    N12, N21 = ref.numeric_jacobians(F, P, S, False, delta=1e-6, narrow=False)
    worst = 0.0
    for k in range(300):
        j12, j21 = hl.edge_jacobians(F, 1, 0, S, c, k)
        for J, Nn in ((j12, N12[k]), (j21, N21[k])):
            worst = max(worst, np.abs(J - Nn).max() / np.abs(J).max())
    out.append("- Analytic Jacobian of the core against central differences (delta = 1e-6) of the restatement's double projection: worst max|dJ| / max|J| "
               "per edge %.3g (bar 1e-5)." % worst)
    d0, runs = T.recovery_runs()
    for mode, name in ((1, "analytic"), (0, "as written")):
        r, d1 = runs[mode]
        out.append("- Recovery, %s: 150 noise-free pairs, start (rotation %.3g rad, |dt| %.3g, ds %.3g) -> end (%.3g, %.3g, %.3g), %d of 150 kept, "
                   "iterations %s." % ((name,) + d0 + d1 + (r["n_inliers"], [int(v) for v in r["iterations"]])))
    return out


def gpu_part(reps):
    import torch
    if not torch.cuda.is_available():
        return None
    torch.cuda.init()
    ctx = api.Context(synth.camera("lafida", F), nfeatures=500, max_batch=1, device=0)
    opt = api.Sim3Optimizer(32, 32 * 150)
    out = ["## Measured on one MI355X and its host CPU", "",
           "One synchronous `cms_sim3_optimize` call, host to host, against `hm_sim3_optimize_host` (one CPU thread) on the same records; N = 150 per job, "
           "outlier share 0.3, median of %d calls after warm-up.  There is no bar on the time." % reps, "",
           "| jobs | jacobian | device call | host core | device per job |", "|---|---|---|---|---|"]
    for mode, name in ((0, "as written"), (1, "analytic")):
        for nj in (1, 8, 32):
            mk = lambda: [api.sim3_opt_job_state(sc.case(900 + j, N=150, outliers=0.3, fix_scale=j % 2), sc.TH2, jacobian=mode) for j in range(nj)]
            st = mk(); arr = api.sim3_opt_jobs(st)
            for _ in range(5):
                opt.optimize(ctx, arr, nj)
            td = []
            for _ in range(reps):
                t0 = time.perf_counter(); opt.optimize(ctx, arr, nj); td.append(time.perf_counter() - t0)
            got = api.sim3_opt_results(arr, st)
            sh = mk(); arh = api.sim3_opt_jobs(sh)
            th = []
            for _ in range(max(5, reps // 5)):
                t0 = time.perf_counter(); rc = hl.H().hm_sim3_optimize_host(F, nj, arh); th.append(time.perf_counter() - t0)
            assert rc == 0 and api.sim3_opt_first_difference(api.sim3_opt_results(arh, sh), got) is None
            out.append("| %d | %s | %.0f us | %.0f us | %.0f us |" % (nj, name, 1e6 * np.median(td), 1e6 * np.median(th), 1e6 * np.median(td) / nj))
    opt.close(); ctx.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not a.cpu_only:      # torch brings its own HIP runtime: it must initialise before the libraries pull in the system one (tests/conftest.py)
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:
            pass
    lines = ["# OptimizeSim3: parity figures and first timings (`tools/prof_sim3_opt.py`)", "",
             "The acceptance bars are bit-equalities (tests/test_sim3_opt_cpu.py, tests/test_gpu_sim3_opt.py); what follows is measured and recorded.", ""]
    lines += cpu_part() + [""]
    g = None if a.cpu_only else gpu_part(a.reps)
    lines += g if g else ["## GPU part not measured in this run"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
