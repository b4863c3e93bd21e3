"""Writes tests/golden/init_v1.npz: the inputs of a few Initializer jobs and what the host build of cms_init_core.h returns for them.  The file pins the
operation order of the core: run this only when the core's definition changes on purpose.

    python tests/golden/make_init_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
IN_KEYS = ("keys1", "rays1", "keys2", "rays2", "matches12", "draws")
OUT_SCALARS = ("status", "best_iteration", "n_inliers", "winner")
OUT_KEYS = ("score", "nGood", "parallax", "R21", "t21", "p3d", "triangulated")


def state_from(z, j):
    from cubemapslam_amd import api
    pr = {k: z["in%d_%s" % (j, k)] for k in IN_KEYS}
    return api.init_job_state(pr, pr["draws"], sigma=float(z["in%d_sigma" % j]))


def result_from(z, j):
    return dict([(k, int(z["out%d_%s" % (j, k)])) for k in OUT_SCALARS] + [(k, z["out%d_%s" % (j, k)]) for k in OUT_KEYS])


def main():
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import init_cases as ic
    import init_hostlib as hl
    from cubemapslam_amd import api, synth
    cf = hl.cos_fov(synth.camera("lafida", ic.F))
    probs = [ic.problem(3, N=60), ic.problem(0, N=200, noise=1.0, outliers=0.3), ic.problem(3, N=70, baseline=0.0), ic.problem(4, N=50, outliers=0.9),
             ic.problem(6, N=90, noise=0.3, outliers=0.1)]
    out = dict(count=len(probs), F=ic.F, cos_fov=np.float32(cf))
    states = []
    for j, pr in enumerate(probs):
        d = ic.draws(700 + j, pr["N"], 200 if j == 1 else 25)
        for k in IN_KEYS[:-1]:
            out["in%d_%s" % (j, k)] = pr[k]
        out["in%d_draws" % j] = d; out["in%d_sigma" % j] = np.float32(1.0)
        states.append(api.init_job_state(pr, d))
    rc, res = hl.two_view_host(ic.F, cf, states)
    assert rc == 0
    for j, r in enumerate(res):
        for k, v in r.items():
            out["out%d_%s" % (j, k)] = v
    np.savez_compressed(os.path.join(HERE, "init_v1.npz"), **out)
    print([r["status"] for r in res])


if __name__ == "__main__":
    main()
