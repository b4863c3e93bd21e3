"""class Sim3Solver of cubemapslam_amd/host/cubemap_hot_path.h without a GPU (engine HOST_CORE: the host build of cms_sim3_core.h): the constructor's
filtering and order (Sim3Solver.cpp:66-127) on key frames with missing, bad, index-less and unprojectable map points on either side, Rcw Xw + tcw,
mvnMaxError, SetRansacParameters, the draws iterate() asks for, vbInliers expanded through mvnIndices1 to size mN1 and GetEstimatedRotation /
Translation / Scale -- against hm_sim3_iterate_host on the job the constructor should have made."""
import numpy as np

import sim3_cases as sc
import sim3_hostlib as hl
from cubemapslam_amd import api


def expected(job, n1, kept, calls, draws, fix_scale, **par):
    mx = api.sim3_ransac_parameters(len(kept), par.get("probability", 0.99), par.get("min_inliers", 20), par.get("max_iterations", 300))
    st = api.sim3_job_state(dict(job, fix_scale=int(fix_scale), min_inliers=par.get("min_inliers", 20), max_its=mx), calls[0], [])
    draws = np.asarray(draws, np.int32).ravel()
    used = 0
    for n_it in calls:
        H = max(mx - st["iterations"], n_it) if len(kept) >= st["min_inliers"] else 0
        st["n_iterations"] = n_it; st["draws"] = draws[used:used + 3 * H].copy(); used += 3 * H
        rc, res = hl.iterate_host(sc.F, [st])
        assert rc == 0
        r = res[0]
        if r["status"] or r["no_more"]:
            break
        st.update(iterations=r["iterations"], best_inliers=r["best_inliers"])
        for k in ("best_R", "best_t", "best_T12", "best_s"):
            st[k] = r[k].copy()
    vb = np.zeros(n1, np.uint8); vb[kept[r["inliers"].astype(bool)]] = 1
    return r, vb, mx, used


def test_constructor_filtering_and_inlier_expansion():
    for fix_scale in (False, True):
        camd, kf1, kf2, m12, kept = hl.mirror_case(fix_scale=fix_scale)
        n1 = len(m12)
        job = hl.mirror_job(kf1, kf2, m12, kept)
        assert sc.in_a_face(job["x3dc1"]).all() and sc.in_a_face(job["x3dc2"]).all()
        for calls in ([5, 5, 5], [300]):
            draws = sc.draws(8, len(kept), 1000)
            got = hl.mirror(1, camd, kf1, kf2, m12, fix_scale, calls, draws)
            assert got["N"] == len(kept) == 61 and np.array_equal(got["indices1"], kept)      # every kind of dropped match left out, key-point order kept
            assert np.array_equal(got["x3dc1"].view(np.uint32), job["x3dc1"].view(np.uint32)) and np.array_equal(got["x3dc2"].view(np.uint32), job["x3dc2"].view(np.uint32))
            r, vb, mx, used = expected(job, n1, kept, calls, draws, fix_scale)
            assert got["max_its"] == mx and got["draws_used"] == used                       # the whole call's draws are made first
            assert r["status"] == 1 and got["found"] == 1 and got["no_more"] == r["no_more"] and got["n_inliers"] == r["n_inliers"] and got["iterations"] == r["iterations"]
            assert len(got["vbInliers"]) == n1 and np.array_equal(got["vbInliers"], vb) and vb.sum() == r["n_inliers"] > 20
            T = got["T12"]
            assert np.array_equal(T[:3].ravel().view(np.uint32), r["T12"].view(np.uint32)) and list(T[3]) == [0, 0, 0, 1]
            assert np.array_equal(got["R"], r["best_R"]) and np.array_equal(got["t"], r["best_t"]) and np.array_equal(got["s"], r["best_s"])
            assert (got["s"][0] == 1.0) == fix_scale


def test_mirror_exhausts_and_too_few():
    camd, kf1, kf2, m12, kept = hl.mirror_case(seed=22)
    job = hl.mirror_job(kf1, kf2, m12, kept)
    par = dict(probability=0.99, min_inliers=len(kept) - 1, max_iterations=12)      # nobody passes: empty Mat, bNoMore
    draws = sc.draws(4, len(kept), 40)
    got = hl.mirror(1, camd, kf1, kf2, m12, False, [5, 5, 5], draws, **par)
    r, vb, mx, used = expected(job, len(m12), kept, [5, 5, 5], draws, False, **par)
    assert got["found"] == 0 and got["no_more"] == 1 and not got["vbInliers"].any() and got["iterations"] == r["iterations"] == mx and got["draws_used"] == used
    assert np.array_equal(got["R"], r["best_R"]) and np.array_equal(got["s"], r["best_s"])
    # too few correspondences: bNoMore at once, no draw made
    few = m12.copy(); few[kept[6:]] = -1
    got = hl.mirror(1, camd, kf1, kf2, few, False, [5], draws)
    assert got["N"] == 6 and got["no_more"] == 1 and got["found"] == 0 and got["draws_used"] == 0
