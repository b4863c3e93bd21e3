"""cms_sim3_iterate on the device against hm_sim3_iterate_host (the host build of the same core, cubemapslam_amd/csrc/cms_sim3_core.h) on the same job
records: status, no_more, n_inliers, iterations, iterations_run, best_inliers, both masks, best_R, best_t, best_s, best_T12 and T12 are equal bit
for bit -- every operation of the core is IEEE-rounded on both sides, so any difference is a finding."""
import numpy as np
import pytest

import sim3_cases as sc
import sim3_hostlib as hl
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu
F = sc.F
MAX_JOBS = 12


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(synth.camera("lafida", F), nfeatures=500, max_batch=1, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def solver():
    s = api.Sim3Solver(max_jobs=MAX_JOBS, max_corr_total=4096, max_hyp_total=2048, device=0)
    yield s
    s.close()


def both(ctx, solver, make_states):
    """The same records through the host loop and through the device; returns (host results, device results)"""
    hs, ds = make_states(), make_states()
    rc, want = hl.iterate_host(F, hs)
    assert rc == 0
    return want, solver.run(ctx, ds)


def same(want, got):
    assert len(want) == len(got)
    diff = api.sim3_first_difference(want, got)
    assert diff is None, diff


def state(seed, N, n_iterations, outliers=0.35, min_inliers=20, max_its=300, **kw):
    pr = sc.problem(seed, N=N, outliers=outliers, min_inliers=min_inliers, max_its=max_its, **kw)
    H = max(max_its, n_iterations) if N >= min_inliers else 0
    return api.sim3_job_state(pr, n_iterations, sc.draws(seed + 1000, N, H) if H else [])


def test_many_jobs_one_call(ctx, solver):
    """Sizes on both sides of one mask word and of the wavefront, a job below min_inliers, 300 hypotheses in one job (several chunks of the replay's
    prefix maximum), both values of fix_scale; accepted, exhausted-with-a-best and empty results in one call"""
    def make():
        out = [state(40 + j, N, 5, fix_scale=j % 2) for j, N in enumerate((20, 21, 63, 64, 65, 128, 129, 257))]
        out.append(state(60, 7, 5))                                                    # below min_inliers: bNoMore, nothing else
        out.append(state(61, 25, 300, outliers=0.3))                                   # never passes 20: all 300 walked, a best is carried out
        out.append(state(62, 150, 300, outliers=0.5, min_inliers=40, fix_scale=1))
        return out
    want, got = both(ctx, solver, make)
    same(want, got)
    assert any(w["status"] == 1 for w in want)
    assert want[8]["no_more"] == 1 and want[8]["status"] == 0 and want[8]["iterations"] == 0 and want[8]["best_inliers"] == 0
    assert want[9]["status"] == 0 and want[9]["no_more"] == 1 and want[9]["iterations"] == 300 and want[9]["best_inliers"] > 3


def test_exhaustion(ctx, solver):
    """min_inliers = N - 1 on N = 200: all 300 hypotheses are computed and walked"""
    want, got = both(ctx, solver, lambda: [state(70, 200, 300, outliers=0.4, min_inliers=199)])
    same(want, got)
    assert want[0]["iterations"] == 300 and want[0]["iterations_run"] == 300 and want[0]["status"] == 0 and want[0]["no_more"] == 1 and want[0]["best_inliers"] > 20


def test_hand_built_loop_cases(ctx, solver):
    """The tie (>= replaces: the second of two equal counts is the best), exactly min_inliers (the best, not accepted), a carried-in best with a
    higher count (stays) and with the same count (replaced and accepted)"""
    n_in, n_out = 12, 8
    N = n_in + n_out
    pr = sc.exact_problem(5, n_in, n_out)
    t1, t2, bad = (0, 1, 2), (3, 4, 5), (0, n_in, n_in + 1)
    mask = np.zeros(N, np.uint8); mask[:6] = 1; mask[n_in:n_in + 7] = 1
    mask12 = mask.copy(); mask12[0] = 0
    carried = dict(best_inliers=13, best_mask=mask, best_T12=np.arange(12), best_R=np.arange(9), best_t=np.arange(3), best_s=2.5, iterations=4)

    def make():
        return [api.sim3_job_state(dict(pr, min_inliers=15, max_its=2), 2, sc.draws_for([t1, t2], N)),
                api.sim3_job_state(dict(pr, min_inliers=n_in, max_its=3), 3, sc.draws_for([bad, t1, bad], N)),
                api.sim3_job_state(dict(pr, min_inliers=n_in - 1, max_its=3), 3, sc.draws_for([bad, t1, bad], N)),
                api.sim3_job_state(dict(pr, min_inliers=10, max_its=6, **carried), 2, sc.draws_for([t1, t2], N)),
                api.sim3_job_state(dict(pr, min_inliers=10, max_its=6, **dict(carried, best_inliers=12, best_mask=mask12)), 2, sc.draws_for([t1, t2], N))]
    want, got = both(ctx, solver, make)
    same(want, got)
    g2 = hl.compute(pr["x3dc1"][list(t2)], pr["x3dc2"][list(t2)])
    assert want[0]["best_inliers"] == n_in and np.array_equal(got[0]["best_T12"], g2["T12"].ravel())
    assert [w["status"] for w in want] == [0, 0, 1, 0, 1] and want[1]["best_inliers"] == n_in and want[3]["best_inliers"] == 13 and np.array_equal(got[3]["best_mask"], mask)


def test_inlier_sweep_word_counts(ctx, solver):
    """The inlier sweep (cms_ransac_mask_sweep) in k_sim3_hypotheses: 1, 1, 2, 3 and 5 mask words in one call (N = 63, 64, 65, 129, 257), exact
    correspondences plus far outliers, 6 to 10 hypotheses per job; hypotheses with an outlier among the three pairs come before the accepted one"""
    def make():
        out = []
        for j, N in enumerate((63, 64, 65, 129, 257)):
            pr = sc.exact_problem(206 + j, N - N // 5, N // 5)
            pr.update(min_inliers=N // 2, max_its=6 + j)
            out.append(api.sim3_job_state(pr, 6 + j, sc.draws(306 + j, N, 6 + j)))
        return out
    want, got = both(ctx, solver, make)
    assert [w["status"] for w in want] == [1] * 5 and [w["iterations_run"] for w in want] == [3, 2, 1, 4, 2]
    assert [w["n_inliers"] for w in want] == [N - N // 5 for N in (63, 64, 65, 129, 257)]
    same(want, got)


def test_two_calls_equal_one(ctx, solver):
    def base():
        return [state(90, 25, 40, outliers=0.3, max_its=40), state(91, 130, 40, min_inliers=129, max_its=40)]      # nothing is ever accepted: the state is carried
    r_one = solver.run(ctx, base())
    first = base()
    for s in first:
        s["n_iterations"] = 10
    r1 = solver.run(ctx, first)
    second = base()
    for s, r in zip(second, r1):
        assert r["iterations"] == 10 and r["no_more"] == 0
        s.update(iterations=r["iterations"], best_inliers=r["best_inliers"], best_mask=r["best_mask"].copy(), best_s=r["best_s"].copy(), draws=s["draws"][30:].copy(), n_iterations=30,
                 **{k: r[k].copy() for k in ("best_R", "best_t", "best_T12")})
    r2 = solver.run(ctx, second)
    assert all(r["iterations"] == 40 and r["no_more"] == 1 for r in r2)
    same(r_one, [dict(b, iterations_run=a["iterations_run"]) for a, b in zip(r_one, r2)])
    rc, want = hl.iterate_host(F, base())
    same(want, r_one)


def test_single_job(ctx, solver):
    want, got = both(ctx, solver, lambda: [state(95, 77, 5)])
    same(want, got)


def test_max_jobs_jobs(ctx, solver):
    want, got = both(ctx, solver, lambda: [state(100 + j, 30 + 9 * j, 5, outliers=0.3 + 0.02 * j) for j in range(MAX_JOBS)])
    same(want, got)
    assert sum(w["status"] for w in want) >= MAX_JOBS // 2


def test_degenerate_inputs_flow_through(ctx, solver):
    """Identical points, all-zero points, NaN and inf coordinates: nothing traps or hangs, and the device still equals the host (NaN bits included)"""
    def make():
        out = []
        for j in range(4):
            pr = sc.problem(120 + j, N=24, outliers=0.0, min_inliers=8, max_its=12)
            if j == 0:
                pr["x3dc1"][:] = pr["x3dc1"][0]; pr["x3dc2"][:] = pr["x3dc2"][0]
            elif j == 1:
                pr["x3dc1"][:] = 0; pr["x3dc2"][:] = 0
            elif j == 2:
                pr["x3dc1"][3] = np.nan; pr["x3dc2"][5] = np.inf
            else:
                pr["x3dc1"][:12] = pr["x3dc1"][0] + np.arange(12, dtype=np.float32)[:, None] * (pr["x3dc1"][1] - pr["x3dc1"][0]) / 8      # collinear
            out.append(api.sim3_job_state(pr, 12, sc.draws(130 + j, 24, 12)))
        return out
    want, got = both(ctx, solver, make)
    same(want, got)


def test_refused_before_anything_is_enqueued(ctx, solver):
    pr = sc.problem(1, N=30, outliers=0.2, min_inliers=10, max_its=5)
    d = sc.draws(2, 30, 5)

    def rc_of(st):
        return api.lib().cms_sim3_iterate(solver.h, ctx.h, 1, api.sim3_jobs([st]))
    e = d.copy(); e[3, 0] = 30
    assert rc_of(api.sim3_job_state(pr, 5, e)) == -1
    e = d.copy(); e[4, 2] = 28
    assert rc_of(api.sim3_job_state(pr, 5, e)) == -1
    assert rc_of(api.sim3_job_state(pr, 5, d[:4])) == -1
    assert rc_of(api.sim3_job_state(dict(pr, best_inliers=2), 5, d)) == -1
    assert rc_of(api.sim3_job_state(dict(pr, min_inliers=2), 5, d)) == -1
    assert rc_of(api.sim3_job_state(dict(pr, max_its=(1 << 20) + 1), 5, d)) == -1
    big = sc.problem(3, N=5000, min_inliers=10, max_its=2)
    assert rc_of(api.sim3_job_state(big, 2, sc.draws(4, 5000, 2))) == -1                       # above the handle's correspondences
    many = dict(pr, max_its=3000)
    assert rc_of(api.sim3_job_state(many, 3000, sc.draws(5, 30, 3000))) == -1                  # above the handle's hypotheses
    states = [api.sim3_job_state(pr, 5, d) for _ in range(MAX_JOBS + 1)]
    assert api.lib().cms_sim3_iterate(solver.h, ctx.h, MAX_JOBS + 1, api.sim3_jobs(states)) == -1      # above the handle's jobs
    assert rc_of(api.sim3_job_state(pr, 5, d)) == 0


def test_mirror_class_on_the_device():
    """class Sim3Solver (cubemap_hot_path.h) with its default engine, the device, against the same class over the host build of the core"""
    camd, kf1, kf2, m12, kept = hl.mirror_case()
    for seed, its in ((8, [5, 5, 5]), (3, [300])):
        draws = sc.draws(seed, len(kept), 900)
        a = hl.mirror(1, camd, kf1, kf2, m12, False, its, draws)
        b = hl.mirror(0, camd, kf1, kf2, m12, False, its, draws)
        assert a["found"] == 1 and a["n_inliers"] > 20
        assert api.sim3_first_difference([a], [b]) is None
