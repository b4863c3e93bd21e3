"""The references of tests/test_gpu_global_ba.py, checked without a device.

1. tests/npref_global_ba.py restates optimize() of oracle/orc_ba.cpp; with the kernel (and the oracle's width, sqrt(5.991)) it must reproduce
   orc.ba_run(prob, its=(N, 0)): identical iteration counts, chi2 within 1e-6 relative, every block within the project's bar.  Held on every
   case of the GPU tests, not only on two: the GPU tests use npref at BundleAdjustment's own width, sqrt(5.99) (Optimizer.cpp:497), where the
   oracle cannot follow (its width is LocalBundleAdjustment's; the width alone moves chi2 by 3e-5 .. 5e-5 relative and points by up to 7e-3 of
   their update on these cases, measured below).
2. Every input of the GPU tests is tame: the reference against itself under a 1e-12 m perturbation of the points stays within the bar
   (strict cases) or cascades on points only (counted cases).  Without the kernel this decides which windows the GPU test may use.
3. Optimizer::CollectGlobalBA against a literal restatement of Optimizer.cpp:480-568."""
import numpy as np
import pytest

import gba_cases as g
import npref_global_ba as npref

ROBUST = g.STRICT + g.CASCADE


@pytest.mark.parametrize("name", ROBUST)
def test_npref_reproduces_the_oracle(name):
    prob = g.problem(name)
    w = g.oracle_robust(name)
    r = g.npref_run(name, True, g.ROBUST_ITS, npref.DELTA_LOCAL)
    assert w["rc"] == 0 and r["iterations_done"] == w["stats"].iterations_done[0]
    rel = abs(r["chi2_final"] - w["stats"].chi2_final[0]) / abs(w["stats"].chi2_final[0])
    pert = g.oracle_robust(name, perturb=True) if name in g.CASCADE else None
    worst, cascaded = g.close_or_cascade(prob, r, w, pert, tag=name)
    print("%s: iterations %d chi2 rel %.3g worst block %.3g cascaded %s" % (name, r["iterations_done"], rel, worst, cascaded))
    assert rel <= 1e-6
    assert abs(r["chi2_initial"] - w["stats"].chi2_initial[0]) <= 1e-9 * abs(w["stats"].chi2_initial[0])
    assert abs(r["lambda_final"] - w["stats"].lambda_final[0]) <= 1e-6 * abs(w["stats"].lambda_final[0])


def test_kernel_width_matters():
    """why the oracle cannot be the GPU tests' reference: sqrt(5.99) against sqrt(5.991) alone is beyond the bar"""
    w = g.oracle_robust("K33")
    r = g.npref_run("K33", True, g.ROBUST_ITS)
    rel = abs(r["chi2_final"] - w["stats"].chi2_final[0]) / abs(w["stats"].chi2_final[0])
    t, q, p = g.block_errors(g.problem("K33"), r["poses"], r["points"], w["poses"], w["points"])
    print("K33, width sqrt(5.99) against the oracle's sqrt(5.991): chi2 rel %.3g, worst key frame %.3g, worst point %.3g" % (rel, max(t.max(), q.max()), p.max()))
    assert rel > 1e-6 and p.max() > g.TOL


def _self(name, robust, its):
    prob = g.problem(name)
    a = g.npref_run(name, robust, its)
    b = g.npref_run(name, robust, its, perturb=True)
    assert a["iterations_done"] == b["iterations_done"]
    t, q, p = g.block_errors(prob, b["poses"], b["points"], a["poses"], a["points"])
    print("%s robust %d: reference against itself: key frames %.3g points %.3g (%d beyond the bar)" % (name, robust, max(t.max(), q.max()), p.max(), int((p > g.TOL).sum())))
    return float(max(t.max(), q.max())), float(p.max())


@pytest.mark.parametrize("name", g.STRICT)
def test_strict_robust_cases_are_tame(name):
    kf, pt = _self(name, True, g.ROBUST_ITS)
    assert kf <= g.TOL and pt <= g.TOL


@pytest.mark.parametrize("name", g.CASCADE)
def test_counted_robust_cases_cascade_on_points_only(name):
    kf, pt = _self(name, True, g.ROBUST_ITS)
    assert kf <= 1e-5      # (whether the points cascade is counted, not required)


def test_cases_without_kernel():
    """the GPU test's windows for robust = 0: at least two of the candidates, one with K >= 33, each tame"""
    tame = []
    for name in g.PLAIN_CANDIDATES:
        kf, pt = _self(name, False, g.PLAIN_ITS)
        if kf <= g.TOL and pt <= g.TOL:
            tame.append(name)
    assert set(g.PLAIN_ADMITTED) <= set(tame), (g.PLAIN_ADMITTED, tame)
    assert len(g.PLAIN_ADMITTED) >= 2 and any(g.CASES[n]["K"] >= 33 for n in g.PLAIN_ADMITTED)


def test_collect_global_ba_against_the_restated_loops():
    import gba_hostlib as hl
    m = g.small_map()
    got = hl.collect(m)
    want = hl.collect_restated(m)
    # the map exercises every rule: a bad key frame, a bad map point, an unlisted key frame's observations, low rays, a point without edges, five faces
    assert m["kf_bad"][:m["n_list"]].any() and m["mp_bad"].any() and (m["obs_kf"] >= m["n_list"]).any()
    assert want["not_included"][m["point_without_edges"]] == 1 and want["not_included"].sum() >= 1
    assert sorted(set(want["e_face"].tolist())) == [0, 1, 2, 3, 4]
    assert want["fixed"].sum() == 1 and want["fixed"][0] == 0
    assert len(want["e_pose"]) < len(m["obs_kf"]) and len(want["vertex_mp"]) < len(m["mp_id"])
    for k in ("vertex_kf", "vertex_mp", "fixed", "e_pose", "e_point", "e_face", "not_included", "points", "e_obs", "e_invsig2"):
        assert np.array_equal(got[k], want[k]), k
    assert np.allclose(got["poses"], want["poses"], rtol=0, atol=1e-15), np.abs(got["poses"] - want["poses"]).max()
