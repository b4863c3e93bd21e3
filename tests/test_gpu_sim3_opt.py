"""cms_sim3_optimize on the device against hm_sim3_optimize_host (the host build of the same core, cubemapslam_amd/csrc/cms_sim3_opt_core.h) on the
same job records: n_inliers, keep, the optimised Sim3 (quaternion, t, s), n_correspondences, n_bad and both iteration counts are equal bit for
bit -- every operation of the core is IEEE-rounded on both sides and exp / sin / cos are the core's own, so any difference is a finding.

The kernel keeps the Levenberg state private to thread 0 and not in LDS (cms_sim3_opt_kernels.hip says why); these tests are the guard of that
choice: a binary that is deterministic but not the host's function shows here as different iteration counts."""
import ctypes as C

import numpy as np
import pytest

import sim3_opt_cases as sc
import sim3_opt_hostlib as hl
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu
F = sc.F
SLOTS = 256
SIZES = (0, 9, 10, 11, SLOTS - 1, SLOTS, SLOTS + 1, 2 * SLOTS + 1, 600)
MAX_JOBS = 16
MAX_CORR = 4096


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(synth.camera("lafida", F), nfeatures=500, max_batch=1, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def opt():
    s = api.Sim3Optimizer(max_jobs=MAX_JOBS, max_corr_total=MAX_CORR, device=0)
    yield s
    s.close()


_CASES = {}


def case(seed, N, outliers, fix_scale):
    key = (seed, N, outliers, fix_scale)
    if key not in _CASES:
        _CASES[key] = sc.case(seed, N=N, outliers=outliers, fix_scale=fix_scale)
    return _CASES[key]


def state(seed, N, outliers, fix_scale, mode):
    return api.sim3_opt_job_state(case(seed, N, outliers, fix_scale), sc.TH2, jacobian=mode)


def same(want, got):
    assert len(want) == len(got)
    diff = api.sim3_opt_first_difference(want, got)
    assert diff is None, diff


def host(states):
    rc, want = hl.optimize_host(F, states)
    assert rc == 0, hl.H().hm_sim3_opt_last_reason()
    return want


def test_slots_constant():
    assert hl.H().hm_s3o_slots() == SLOTS


@pytest.mark.parametrize("outliers", (0.0, 0.3))
@pytest.mark.parametrize("fix_scale", (0, 1))
@pytest.mark.parametrize("mode", (api.SIM3_OPT_AS_WRITTEN, api.SIM3_OPT_ANALYTIC))
def test_device_equals_host_core(ctx, opt, mode, fix_scale, outliers):
    """Every size on both sides of the policy's 10 survivors and of the slot count, in one call"""
    make = lambda: [state(300 + N, N, outliers, fix_scale, mode) for N in SIZES]
    want = host(make())
    got = opt.run(ctx, make())
    same(want, got)
    assert want[0]["n_inliers"] == 0 and want[1]["n_inliers"] == 0 and [w["n_correspondences"] for w in want] == list(SIZES)
    assert want[-1]["n_inliers"] >= 300 and want[-1]["iterations"][1] >= 1
    if outliers:
        assert want[-1]["n_bad"] > 60


def mixed_states():
    out = []
    for j, N in enumerate((150, 0, 9, 31, 64, 300, 257, 12, 100, 77, 200, 10, 255, 129, 40, 500)):
        out.append(state(400 + j, N, 0.9 if N == 12 else (0.3 if j % 3 else 0.0), j % 2, (j // 2) % 2))
    return out


def test_sixteen_mixed_jobs_equal_each_alone(ctx, opt):
    """One call with 16 jobs of mixed sizes, modes and fix_scale, with an N == 0 job, one below 10 correspondences and one that loses too many at
    :1061: equal to the host core, and each job equal to the same job alone in a call"""
    want = host(mixed_states())
    got = opt.run(ctx, mixed_states())
    same(want, got)
    assert want[1]["n_correspondences"] == 0 and want[1]["n_inliers"] == 0
    assert want[7]["n_correspondences"] - want[7]["n_bad"] < 10 and want[7]["n_bad"] > 0 and want[7]["n_inliers"] == 0 and want[7]["iterations"][1] == 0
    alone = [opt.run(ctx, [s])[0] for s in mixed_states()]
    same(got, alone)


def test_handle_reuse(ctx, opt):
    """Two different calls on one handle, then the first again: the same bits"""
    a = lambda: [state(500, 300, 0.3, 0, 0), state(501, 40, 0.0, 1, 1)]
    b = lambda: [state(502, 600, 0.3, 1, 0)]
    first = opt.run(ctx, a())
    second = opt.run(ctx, b())
    again = opt.run(ctx, a())
    same(first, again)
    same(host(a()), first)
    same(host(b()), second)


def _refused(ctx, opt, states, arr=None, njobs=None):
    arr = api.sim3_opt_jobs(states) if arr is None else arr
    with pytest.raises(api.CmsError) as e:
        opt.optimize(ctx, arr, len(states) if njobs is None else njobs)
    for q, s in zip(arr, states):      # the records untouched
        assert q.n_inliers == -7 and q.n_correspondences == -7 and q.n_bad == -7 and list(q.iterations) == [-7, -7]
        assert (s["keep"] == 7).all()
    return str(e.value)


def test_error_paths_leave_the_records_untouched(ctx, opt):
    good = lambda: [state(510, 64, 0.3, 0, 0), state(511, 30, 0.0, 0, 1)]
    want = host(good())

    def broken(**kw):
        st = good()
        st[1].update(kw)
        return st
    msgs = []
    st = good(); st[1]["kp2"] = None
    msgs.append(_refused(ctx, opt, st))                                          # a null array
    for th2 in (0.0, -1.0, float("nan"), float("inf")):
        msgs.append(_refused(ctx, opt, broken(th2=th2)))
    for s12 in (0.0, -0.5, float("nan"), float("inf")):
        msgs.append(_refused(ctx, opt, broken(s12=s12)))
    for jac in (-1, 2):
        msgs.append(_refused(ctx, opt, broken(jacobian=jac)))
    for bad_kp in ((10.0, 10.0), (-1.0, F + 5.0), (3.0 * F, F + 1.0), (float("nan"), F + 1.0)):      # a corner block, left of the image, right of it, NaN
        st = good(); st[0]["kp1"][17] = bad_kp
        msgs.append(_refused(ctx, opt, st))
        st = good(); st[1]["kp2"][3] = bad_kp
        msgs.append(_refused(ctx, opt, st))
    msgs.append(_refused(ctx, opt, [state(512, 600, 0.0, 0, 0) for _ in range(7)]))      # 4200 correspondences > MAX_CORR
    msgs.append(_refused(ctx, opt, [state(513, 10, 0.0, 0, 0) for _ in range(MAX_JOBS + 1)]))
    assert all("cms_sim3_optimize" in m for m in msgs), msgs
    with pytest.raises(api.CmsError):
        api._chk(api.lib().cms_sim3_optimize(opt.h, ctx.h, 2, None), "cms_sim3_optimize")
    # njobs == 0 is CMS_OK with no launch, and the next valid call is correct
    opt.optimize(ctx, api.sim3_opt_jobs([]), 0)
    same(want, opt.run(ctx, good()))


@pytest.mark.parametrize("jacobian", (api.SIM3_OPT_AS_WRITTEN, api.SIM3_OPT_ANALYTIC))
def test_mirror_default_engine_equals_host_core(jacobian):
    """Optimizer::OptimizeSim3 of cubemap_hot_path.h with its default engine (the device) against the same class over HOST_CORE: the graph, vpMatches1
    afterwards, the return value and the optimised Sim3, bit for bit"""
    for fix_scale in (False, True):
        camd, kf1, kf2, m12, start = hl.mirror_case(fix_scale=fix_scale)
        want = hl.mirror(1, camd, kf1, kf2, m12, start, sc.TH2, fix_scale, jacobian)
        got = hl.mirror(0, camd, kf1, kf2, m12, start, sc.TH2, fix_scale, jacobian)
        assert want["N"] > 60 and want["n_inliers"] >= 20 and (want["matches1"] != np.asarray(m12)).any()
        for k in want:
            assert np.asarray(want[k]).tobytes() == np.asarray(got[k]).tobytes(), (fix_scale, k)
