"""Regenerates tests/golden/pnp_v1.npz: inputs, draws and the host build's outputs (hm_pnp_iterate_host) of six PnP jobs.

    python tests/golden/make_pnp_golden.py

The outputs are those of cubemapslam_amd/csrc/cms_pnp_core.h as it stands: a change of the order of its operations changes them, and has to
regenerate this file and say so."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pnp_cases as pc      # noqa: E402
import pnp_hostlib as hl    # noqa: E402
from cubemapslam_amd import api      # noqa: E402

IN_KEYS = ("p3d", "p2d", "bearing", "sigma2", "draws", "best_Tcw", "best_mask")
IN_SCALARS = ("th2", "min_inliers", "max_its", "n_iterations", "iterations", "best_inliers")
OUT_KEYS = ("Tcw", "best_Tcw", "inliers", "best_mask")
OUT_SCALARS = ("status", "no_more", "n_inliers", "iterations", "iterations_run", "best_inliers")


def states():
    out = []
    for j, N in enumerate((60, 65, 130)):
        pr = pc.problem(40 + j, N=N, outliers=0.3, noise=1.0)
        mi, mx, _ = api.ransac_parameters(N, 0.99, 10, 35, 4, 0.5)
        pr.update(min_inliers=mi, max_its=mx)
        out.append(api.pnp_job_state(pr, 5, pc.draws(140 + j, N, mx)))
    base = pc.exact_problem(5, 12, 8)
    d = pc.draws(11, 20, 13)
    rng = np.random.default_rng(0)      # a quadruple of inliers that recovers all twelve (not every one does), as iterations 5 and 10
    while True:
        q = [int(v) for v in rng.choice(12, 4, replace=False)]
        one = api.pnp_job_state(dict(base, min_inliers=12, max_its=1), 1, pc.draws_for([q], 20))
        if hl.iterate_host(pc.F, [one])[1][0]["best_inliers"] == 12:
            break
    d[4] = d[9] = pc.draws_for([q], 20)[0]
    mask = np.zeros(20, np.uint8); mask[:6] = 1; mask[12:19] = 1
    out.append(api.pnp_job_state(dict(base, min_inliers=12, max_its=13), 5, d))
    out.append(api.pnp_job_state(dict(base, min_inliers=10, max_its=13, best_inliers=13, best_mask=mask, best_Tcw=np.arange(12)), 5, d))
    pr = pc.problem(120, N=24, outliers=0.0); pr["p3d"][:] = pr["p3d"][0]; pr.update(min_inliers=8, max_its=12)
    out.append(api.pnp_job_state(pr, 5, pc.draws(130, 24, 12)))
    return out


def state_from(z, j):
    """The job state of case j of a loaded pnp_v1.npz"""
    pr = {k: z["in%d_%s" % (j, k)] for k in IN_KEYS if k != "draws"}
    sc = {k: z["in%d_%s" % (j, k)].item() for k in IN_SCALARS}
    pr.update(min_inliers=sc["min_inliers"], max_its=sc["max_its"], iterations=sc["iterations"], best_inliers=sc["best_inliers"])
    return api.pnp_job_state(pr, sc["n_iterations"], z["in%d_draws" % j], th2=sc["th2"])


if __name__ == "__main__":
    st = states()
    d = {"count": np.int32(len(st)), "F": np.int32(pc.F)}
    for j, s in enumerate(st):
        for k in IN_KEYS:
            d["in%d_%s" % (j, k)] = s[k].copy()
        for k in IN_SCALARS:
            d["in%d_%s" % (j, k)] = np.float32(s[k]) if k == "th2" else np.int32(s[k])
    rc, res = hl.iterate_host(pc.F, st)
    assert rc == 0
    for j, r in enumerate(res):
        for k in OUT_KEYS:
            d["out%d_%s" % (j, k)] = r[k]
        for k in OUT_SCALARS:
            d["out%d_%s" % (j, k)] = np.int32(r[k])
    path = os.path.join(HERE, "pnp_v1.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes;", [(r["status"], r["iterations"], r["n_inliers"]) for r in res])
