"""class PnPsolver of cubemapslam_amd/host/cubemap_hot_path.h without a GPU (engine HOST_CORE: the host build of cms_pnp_core.h): the constructor's
filtering and order (PnPsolver.cpp:83-108) on a frame with NULL and bad map points, SetRansacParameters, the draws iterate() asks for, and vbInliers
expanded through mvKeyPointIndices -- against hm_pnp_iterate_host on the job the constructor should have made."""
import numpy as np

import pnp_cases as pc
import pnp_hostlib as hl
from cubemapslam_amd import api


def expected(job, kept, n, n_iterations, draws, **par):
    mi, mx, _ = api.ransac_parameters(len(kept), par.get("probability", 0.99), par.get("min_inliers", 8), par.get("max_iterations", 300), 4, par.get("epsilon", 0.4))
    st = api.pnp_job_state(dict(job, min_inliers=mi, max_its=mx), n_iterations, draws, th2=par.get("th2", 5.991))
    rc, res = hl.iterate_host(pc.F, [st])
    assert rc == 0
    r = res[0]
    vb = np.zeros(n, np.uint8); vb[kept[r["inliers"].astype(bool)]] = 1
    return r, vb, mx


def test_constructor_filtering_and_inlier_expansion():
    camd, frame, mp, bad, pos, kept, job = hl.mirror_case()
    n = len(mp)
    par = dict(probability=0.99, min_inliers=10, max_iterations=40, epsilon=0.5)
    # draws 8: Refine accepts (mRefinedTcw, the refined mask); draws 3: the iterations run out and the best is handed out (mBestTcw, the best mask) --
    # in this frame Refine's first inlier lies behind the front face's image plane, so solve_for_sign mirrors its solve, as in the reference
    for seed, status in ((8, 1), (3, 2)):
        draws = pc.draws(seed, len(kept), 40)
        got = hl.mirror(1, camd, frame, mp, bad, pos, [5], draws, **par)
        assert got["N"] == len(kept) == 61 and np.array_equal(got["key_idx"], kept)          # NULL and bad map points left out, key-point order kept
        r, vb, mx = expected(job, kept, n, 5, draws, **par)
        assert got["draws_used"] == 4 * max(mx, 5)                                             # the whole call's draws are made first
        assert r["status"] == status and got["found"] == 1 and got["no_more"] == r["no_more"] and got["n_inliers"] == r["n_inliers"] and got["iterations"] == r["iterations"]
        assert np.array_equal(got["vbInliers"], vb) and vb.sum() == r["n_inliers"] and not vb[mp < 0].any() and not vb[bad.astype(bool)].any()
        T = got["Tcw"]
        assert np.array_equal(T[:3, :3].ravel().view(np.uint32), r["Tcw"][:9].view(np.uint32)) and np.array_equal(T[:3, 3].view(np.uint32), r["Tcw"][9:].view(np.uint32))
        assert list(T[3]) == [0, 0, 0, 1]

def test_mirror_exhausts_and_reports_the_best():
    camd, frame, mp, bad, pos, kept, job = hl.mirror_case(seed=22)
    par = dict(probability=0.99, min_inliers=len(kept), max_iterations=12, epsilon=0.5)      # nobody passes: empty Mat, bNoMore
    draws = pc.draws(4, len(kept), 12)
    got = hl.mirror(1, camd, frame, mp, bad, pos, [5], draws, **par)
    r, vb, mx = expected(job, kept, len(mp), 5, draws, **par)
    assert mx == 1 and got["found"] == 0 and got["no_more"] == 1 and not got["vbInliers"].any() and got["iterations"] == r["iterations"] == 5
    # too few correspondences: bNoMore at once, no draw made
    few = mp.copy(); few[kept[6:]] = -1
    got = hl.mirror(1, camd, frame, few, bad, pos, [5], draws, probability=0.99, min_inliers=8, max_iterations=300, epsilon=0.4)
    assert got["N"] == 6 and got["no_more"] == 1 and got["found"] == 0 and got["draws_used"] == 0
