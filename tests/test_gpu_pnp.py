"""cms_pnp_iterate on the device against hm_pnp_iterate_host (the host build of the same core, cubemapslam_amd/csrc/cms_pnp_core.h) on the same job
records: status, no_more, n_inliers, iterations, iterations_run, both masks, best_inliers and the 12 + 12 floats are equal bit for bit -- every
operation of the core is IEEE-rounded on both sides, so any difference is a finding."""
import numpy as np
import pytest

import pnp_cases as pc
import pnp_hostlib as hl
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu
F = pc.F
KEYS_I = ("status", "no_more", "n_inliers", "iterations", "iterations_run", "best_inliers")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(synth.camera("lafida", F), nfeatures=500, max_batch=1, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def solver():
    s = api.PnPSolver(max_jobs=16, max_corr_total=4096, max_hyp_total=2048, device=0)
    yield s
    s.close()


def both(ctx, solver, make_states):
    """The same records through the host loop and through the device; returns (host results, device results)"""
    hs, ds = make_states(), make_states()
    rc, want = hl.iterate_host(F, hs)
    assert rc == 0
    arr = api.pnp_jobs(ds)
    solver.iterate(ctx, arr)
    return want, api.pnp_results(arr, ds)


def same(want, got):
    assert len(want) == len(got)
    diff = api.pnp_first_difference(want, got)
    assert diff is None, diff


def noisy_states(sizes, seed0, n_iterations=5, its=35, **kw):
    def make():
        out = []
        for j, N in enumerate(sizes):
            pr = pc.problem(seed0 + j, N=N, outliers=0.3, noise=1.0)
            mi, mx, _ = api.ransac_parameters(N, 0.99, 10, its, 4, 0.5)
            pr.update(min_inliers=mi, max_its=mx, **kw)
            H = max(mx, n_iterations) if N >= mi else 0
            out.append(api.pnp_job_state(pr, n_iterations, pc.draws(seed0 + 100 + j, N, H) if H else []))
        return out
    return make


def test_many_jobs_one_call(ctx, solver):
    """Sizes on both sides of one mask word and of the select workgroup's four waves, a job below min_inliers, more than one workgroup of
    hypotheses; accepted, exhausted-with-a-best and empty results in one call"""
    sizes = [60, 65, 7, 130, 64, 257, 321, 20, 63, 129]
    want, got = both(ctx, solver, noisy_states(sizes, 40))
    same(want, got)
    st = [w["status"] for w in want]
    assert 1 in st and want[2]["no_more"] == 1 and want[2]["status"] == 0, st


def test_exhaustion_paths(ctx, solver):
    """min_inliers nobody can pass (every hypothesis is computed and walked: 300 of them), and a bar that only the best reaches (status 2)"""
    def make():
        out = []
        for j, (N, mi, its) in enumerate(((200, 199, 300), (90, 50, 40), (45, 30, 33))):
            pr = pc.problem(70 + j, N=N, outliers=0.4, noise=0.5)
            pr.update(min_inliers=mi, max_its=its)
            out.append(api.pnp_job_state(pr, 5, pc.draws(170 + j, N, its)))
        return out
    want, got = both(ctx, solver, make)
    same(want, got)
    assert want[0]["iterations"] == 300 and want[0]["status"] == 0 and want[0]["no_more"] == 1


def test_hand_built_loop_cases(ctx, solver):
    """Exact inliers plus far outliers: a best carried in that a weaker hypothesis must not replace (Refine on the best mask), exactly min_inliers
    (qualifies on >=, Refine refused on >), the same count twice (best only on >)"""
    n_in, n_out = 12, 8
    N = n_in + n_out
    base = pc.exact_problem(5, n_in, n_out)
    bad_mask = np.zeros(N, np.uint8); bad_mask[:6] = 1; bad_mask[n_in:n_in + 7] = 1

    def make():
        d = pc.draws(11, N, 13)
        a = api.pnp_job_state(dict(base, min_inliers=10, max_its=13, best_inliers=13, best_mask=bad_mask, best_Tcw=np.arange(12)), 5, d)
        b = api.pnp_job_state(dict(base, min_inliers=n_in, max_its=13), 5, d)
        c = api.pnp_job_state(dict(base, min_inliers=n_in - 1, max_its=13), 5, d)
        e = api.pnp_job_state(dict(base, min_inliers=4, max_its=13), 5, d)
        return [a, b, c, e]
    want, got = both(ctx, solver, make)
    same(want, got)
    assert want[0]["best_inliers"] == 13 and want[0]["status"] == 2 and np.array_equal(want[0]["best_mask"], bad_mask)


def test_inlier_sweep_word_counts(ctx, solver):
    """The inlier sweep (cms_ransac_mask_sweep) in k_pnp_inliers and in the Refine of k_pnp_select, whose four waves take the words w, w + 4, ...:
    1, 1, 2, 3 and 5 mask words in one call (N = 63, 64, 65, 129, 257), exact correspondences plus far outliers, 6 to 10 hypotheses per job.  The
    seeds were chosen with the host loop alone so that Refine is reached, accepted and refused."""
    sizes = (63, 64, 65, 129, 257)

    def make():
        out = []
        for seed0 in (209, 208):
            for j, N in enumerate(sizes):
                pr = pc.exact_problem(seed0 + j, N - N // 5, N // 5)
                pr.update(min_inliers=N // 2, max_its=6 + j)
                out.append(api.pnp_job_state(pr, 5, pc.draws(seed0 + 100 + j, N, 6 + j)))
        return out
    want, got = both(ctx, solver, make)
    st = [w["status"] for w in want]
    # Refine accepted on 2 and 3 words and on 5 (more words than waves); refused on the best of all 10 hypotheses of the first 257 (status 2)
    assert st[2] == 1 and st[3] == 1 and st[9] == 1 and st[4] == 2 and want[4]["iterations_run"] == 10, st
    assert want[0]["status"] == 1 and want[0]["n_inliers"] > want[0]["best_inliers"]      # the refined mask is not the best mask
    same(want, got)


def test_two_calls_equal_one(ctx, solver):
    sizes = [60, 130]
    mk = noisy_states(sizes, 90, its=24)

    def with_bar():
        st = mk()
        for s in st:
            s["min_inliers"] = s["N"]        # nothing is ever accepted: the state is carried
        return st
    one = with_bar()
    arr = api.pnp_jobs(one); solver.iterate(ctx, arr); r_one = api.pnp_results(arr, one)
    first = with_bar()
    for s in first:
        s["max_its"] = 10; s["n_iterations"] = 10; s["draws"] = s["draws"][:40].copy()
    arr = api.pnp_jobs(first); solver.iterate(ctx, arr); r1 = api.pnp_results(arr, first)
    second = with_bar()
    for s, r in zip(second, r1):
        assert r["iterations"] == 10
        s.update(iterations=r["iterations"], best_inliers=r["best_inliers"], best_mask=r["best_mask"].copy(), best_Tcw=r["best_Tcw"].copy(), draws=s["draws"][40:].copy(), n_iterations=1)
    arr = api.pnp_jobs(second); solver.iterate(ctx, arr); r2 = api.pnp_results(arr, second)
    for a, b in zip(r_one, r2):
        b = dict(b, iterations_run=a["iterations_run"])
        same([a], [b])


def test_degenerate_inputs_flow_through(ctx, solver):
    """Four identical points, all-zero points and NaN coordinates: nothing traps or hangs, and the device still equals the host (NaN bits included)"""
    def make():
        out = []
        for j in range(3):
            pr = pc.problem(120 + j, N=24, outliers=0.0)
            if j == 0:
                pr["p3d"][:] = pr["p3d"][0]
            elif j == 1:
                pr["p3d"][:] = 0; pr["bearing"][:] = 0
            else:
                pr["p3d"][3] = np.nan; pr["p2d"][5] = np.inf
            pr.update(min_inliers=8, max_its=12)
            out.append(api.pnp_job_state(pr, 5, pc.draws(130 + j, 24, 12)))
        return out
    want, got = both(ctx, solver, make)
    same(want, got)


def test_refused_before_anything_is_enqueued(ctx, solver):
    pr = pc.problem(1, N=30)
    pr.update(min_inliers=10, max_its=5)
    d = pc.draws(2, 30, 5)

    def rc_of(state):
        arr = api.pnp_jobs([state])
        return api.lib().cms_pnp_iterate(solver.h, ctx.h, 1, arr)
    e = d.copy(); e[3, 0] = 30
    assert rc_of(api.pnp_job_state(pr, 5, e)) == -1
    e = d.copy(); e[4, 3] = 27
    assert rc_of(api.pnp_job_state(pr, 5, e)) == -1
    assert rc_of(api.pnp_job_state(pr, 5, d[:4])) == -1
    assert rc_of(api.pnp_job_state(pr, 5, d, min_set=5)) == -3
    assert rc_of(api.pnp_job_state(dict(pr, best_inliers=2), 5, d)) == -1
    big = pc.problem(3, N=5000); big.update(min_inliers=10, max_its=2)
    assert rc_of(api.pnp_job_state(big, 1, pc.draws(4, 5000, 2))) == -1            # above the handle's correspondences
    many = dict(pr, max_its=3000)
    assert rc_of(api.pnp_job_state(many, 1, pc.draws(5, 30, 3000))) == -1           # above the handle's hypotheses
    assert rc_of(api.pnp_job_state(pr, 5, d)) == 0


def test_golden_cases_on_the_device(ctx, solver):
    """The recorded host outputs of tests/golden/pnp_v1.npz, all six jobs in one call"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_pnp_golden", os.path.join(root, "tests", "golden", "make_pnp_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    z = np.load(os.path.join(root, "tests", "golden", "pnp_v1.npz"))
    st = [G.state_from(z, j) for j in range(int(z["count"]))]
    arr = api.pnp_jobs(st)
    solver.iterate(ctx, arr)
    got = api.pnp_results(arr, st)
    want = [dict([(k, int(z["out%d_%s" % (j, k)])) for k in G.OUT_SCALARS] + [(k, z["out%d_%s" % (j, k)]) for k in G.OUT_KEYS]) for j in range(len(st))]
    same(want, got)


@pytest.fixture(scope="module")
def frame_row():
    """A context whose row 0 holds an extracted frame, and two PnP jobs on it with different mvKeyPointIndices: (context, key-point count,
    states(frames) -> fresh job records, for cms_pnp_iterate_frames or with the row's data fetched to the host)"""
    camd = synth.camera("lafida", 150)
    c = api.Context(camd, nfeatures=800, max_batch=1, device=0)
    try:
        c.set_mask(synth.cubemap_valid_mask(camd, erode=5, band=30))
        k, _ = c.remap_extract(synth.texture(camd["Ih"], camd["Iw"], 3))
        rays = c.fetch_rays(0)
        n = len(k)
        assert n > 300 and len(rays) == n
        sigma2_levels = np.array(c.geom.sigma2[:8], np.float32)

        def states(frames):
            out = []
            for j, N in enumerate((200, 77)):
                r = np.random.default_rng(50 + j)
                idx = np.sort(r.choice(n, N, replace=False)).astype(np.int32)
                R, t = pc.random_pose(r)
                ray = rays[idx].astype(np.float64)
                Xc = ray / np.linalg.norm(ray, axis=1, keepdims=True) * r.uniform(1.5, 8.0, (N, 1))
                Xw = (Xc - t) @ R
                Xw[r.choice(N, N // 4, replace=False)] += r.normal(0, 2.0, (N // 4, 3))          # outliers
                pr = dict(p3d=Xw.astype(np.float32), p2d=np.stack([k["x"][idx], k["y"][idx]], 1), bearing=rays[idx], sigma2=sigma2_levels[k["octave"][idx]])
                pr["min_inliers"], pr["max_its"], _ = api.ransac_parameters(N, 0.99, 10, 40, 4, 0.5)
                s = api.pnp_job_state(pr, 5, pc.draws(60 + j, N, pr["max_its"]))
                if frames:
                    s.update(kp_idx=idx, b=0, n=n, p2d=np.zeros((N, 2), np.float32), bearing=np.zeros((N, 3), np.float32), sigma2=np.zeros(N, np.float32))
                out.append(s)
            return out
        yield c, n, states
    finally:
        c.close()


def test_iterate_frames_gathers_from_the_resident_row(frame_row):
    """cms_pnp_iterate_frames (key point, key ray and level sigma2 gathered on the device from the row the extractor left) against cms_pnp_iterate and
    the host loop on the same data fetched to the host: two jobs on one row with different mvKeyPointIndices"""
    c, n, states = frame_row
    F150 = 150
    rc, want = hl.iterate_host(F150, states(False))
    assert rc == 0
    S = api.PnPSolver(4, 1024, 512)
    try:
        same(want, S.run(c, states(False)))
        got = S.run(c, states(True), frames=True)
        same(want, got)
        # refused before anything is enqueued: an index at the row's count, a row beyond the batch
        bad = states(True); bad[0]["kp_idx"] = bad[0]["kp_idx"].copy(); bad[0]["kp_idx"][5] = n
        assert api.lib().cms_pnp_iterate_frames(S.h, c.h, 2, api.pnp_jobs(bad)) == -1
        bad = states(True); bad[1]["b"] = 1
        assert api.lib().cms_pnp_iterate_frames(S.h, c.h, 2, api.pnp_jobs(bad)) == -1
    finally:
        S.close()


def test_handle_reuse(ctx, frame_row):
    """One handle through a large call, a small one and the large one again on its own stream, with calls on a frame context's stream in between (the
    same pair of blocks used from the other stream): the blocks are grown once and reused, and every result is that of a fresh handle"""
    fc, _, frame_states = frame_row
    large = noisy_states([60, 65, 7, 130, 64, 257, 321, 20, 63, 129], 40)
    small = noisy_states([20], 47)
    calls = [(ctx, large, False), (fc, lambda: frame_states(True), True), (ctx, small, False), (fc, lambda: frame_states(True), True), (ctx, large, False)]

    def fresh(c, make, frames):
        S = api.PnPSolver(16, 4096, 2048)
        try:
            return S.run(c, make(), frames=frames)
        finally:
            S.close()
    want = [fresh(*call) for call in calls[:3]]
    want += [want[1], want[0]]
    S = api.PnPSolver(16, 4096, 2048)
    try:
        for (c, make, frames), w in zip(calls, want):
            same(w, S.run(c, make(), frames=frames))
    finally:
        S.close()


def test_mirror_class_on_the_device():
    """class PnPsolver (cubemap_hot_path.h) with its default engine, the device, against the same class over the host build of the core"""
    camd, frame, mp, bad, pos, kept, job = hl.mirror_case()
    par = dict(probability=0.99, min_inliers=10, max_iterations=40, epsilon=0.5)
    for seed in (8, 3):
        draws = pc.draws(seed, len(kept), 40)
        a = hl.mirror(1, camd, frame, mp, bad, pos, [5], draws, **par)
        b = hl.mirror(0, camd, frame, mp, bad, pos, [5], draws, **par)
        assert a["found"] == 1
        assert api.pnp_first_difference([a], [b]) is None
