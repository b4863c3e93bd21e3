"""cms_init_two_view on the device against hm_init_two_view_host (the host build of the same core, cubemapslam_amd/csrc/cms_init_core.h) on the same job
records: status, R21, t21, p3d, triangulated and every diagnostic (best_iteration, score, n_inliers, the four nGood, the four parallaxes, winner) are
equal bit for bit -- every operation of the core is IEEE-rounded on both sides, so any difference is a finding."""
import numpy as np
import pytest

import init_cases as ic
import init_hostlib as hl
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu
F = ic.F
CAMD = synth.camera("lafida", F)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(CAMD, nfeatures=500, max_batch=1, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ini():
    s = api.TwoViewInitializer(max_jobs=16, max_matches_total=4096, max_keys1_total=8192, max_hyp_total=4096, device=0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def cosfov():
    return hl.cos_fov(CAMD)


def both(ctx, ini, cosfov, make_states):
    """The same records through the host loop and through the device; returns (host results, device results)"""
    hs, ds = make_states(), make_states()
    rc, want = hl.two_view_host(F, cosfov, hs)
    assert rc == 0
    return want, ini.run(ctx, ds)


def same(want, got):
    assert len(want) == len(got)
    diff = api.init_first_difference(want, got)
    assert diff is None, diff


SIZES = (8, 9, 63, 64, 65, 100, 129, 257, 700)


def sized_states(iterations, seed0=300):
    def make():
        out = []
        for j, N in enumerate(SIZES):
            pr = ic.problem(seed0 + j, N=N, extra1=3 + 5 * j, extra2=40 - 3 * j, noise=0.5 if j % 2 else 0.0, outliers=0.2 if N >= 63 else 0.0)
            out.append(api.init_job_state(pr, ic.draws(seed0 + 50 + j, N, iterations)))
        return out
    return make


def test_many_jobs_one_call(ctx, ini, cosfov):
    """Sizes on both sides of one mask word, of the select workgroup's 256 threads and of the 50th cosine; n1 != n2 != N per job; 200 iterations, i.e.
    more than one workgroup of hypotheses per job; then the same jobs with 1 and with 7 iterations"""
    want, got = both(ctx, ini, cosfov, sized_states(200))
    same(want, got)
    st = [w["status"] for w in want]
    assert 1 in st and 0 in st, st
    for its in (1, 7):
        want, got = both(ctx, ini, cosfov, sized_states(its, 340))
        same(want, got)


def decision_states():
    ok = ic.problem(3, N=120)
    rot = ic.problem(3, N=120, baseline=0.0)
    few = ic.problem(3, N=100, outliers=0.95)
    far = ic.problem(9, N=150, noise=1.5, baseline=0.02, depth=(30.0, 31.0))     # noisy points far away over a tiny baseline
    low = ic.problem(9, N=150, baseline=0.01, depth=(6.0, 8.0))                  # a clear winner without parallax
    return [api.init_job_state(p, ic.draws(5 + i, p["N"], 200)) for i, p in enumerate((ok, rot, few, far, low))]


def path_of(r):
    """The return path of ReconstructE (:305-375) a result took, from its diagnostics"""
    g = r["nGood"]
    if (g > 0.7 * g.max()).sum() > 1:
        return "similar"
    if g.max() < max(int(0.9 * r["n_inliers"]), 50):
        return "few"
    return "ok" if r["status"] == 1 else "parallax"


def test_decision_paths_in_one_call(ctx, ini, cosfov):
    """Success, pure rotation (two hypotheses reconstruct alike: no clear winner), too few good points and a clear winner without parallax in one call"""
    want, got = both(ctx, ini, cosfov, decision_states)
    same(want, got)
    assert [path_of(w) for w in want] == ["ok", "similar", "few", "few", "parallax"]


def boundary_states(cosfov):
    """Jobs whose best hypothesis has nGood of 50, 51 and 52: the match list of a noise-free problem trimmed until the host core reports them"""
    base = ic.problem(11, N=80)
    found = {}
    for keep in range(50, 70):
        pr = ic.trim(base, keep)
        st = api.init_job_state(pr, ic.draws(12, keep, 20))
        rc, res = hl.two_view_host(F, cosfov, [st])
        assert rc == 0
        found.setdefault(int(res[0]["nGood"].max()), keep)
    assert all(k in found for k in (50, 51, 52)), found
    return lambda: [api.init_job_state(ic.trim(base, found[k]), ic.draws(12, found[k], 20)) for k in (50, 51, 52)]


def test_selected_cosine_at_its_boundary(ctx, ini, cosfov):
    """min(50, nGood-1): nGood = 50 reads the last element, 51 the last, 52 the one before the last"""
    make = boundary_states(cosfov)
    want, got = both(ctx, ini, cosfov, make)
    same(want, got)
    assert [int(w["nGood"].max()) for w in want] == [50, 51, 52]


def degenerate_states():
    out = []
    base = ic.problem(21, N=90)
    at = np.flatnonzero(base["matches12"] >= 0)
    sets = [list(range(8 * i, 8 * i + 8)) for i in range(6)]           # matches 0..47 are drawn, 48.. never
    d = ic.draws_for(sets, 90)
    a = dict(base, rays1=base["rays1"].copy()); a["rays1"][at[3]] = np.nan           # inside the first set
    b = dict(base, rays2=base["rays2"].copy()); b["rays2"][base["matches12"][at[70]]] = np.nan      # outside every set
    c = dict(base, rays1=base["rays1"].copy()); c["rays1"][at[10]] = 0.0             # a zero ray, drawn
    e = dict(base, keys2=base["keys1"].copy(), rays2=base["rays1"].copy(), matches12=np.where(base["matches12"] >= 0, np.arange(len(base["matches12"])), -1))
    for p in (a, b, c, e):
        out.append(api.init_job_state(p, d))
    return out


def test_non_finite_and_degenerate_inputs(ctx, ini, cosfov):
    """A NaN ray inside a drawn set, one outside every set, a zero ray, two identical views: the call returns, and the bits are the host core's"""
    want, got = both(ctx, ini, cosfov, degenerate_states)
    same(want, got)
    assert want[3]["status"] == 0


def test_refused_before_anything_is_enqueued(ctx, ini, cosfov):
    pr = ic.problem(31, N=40)
    d = ic.draws(32, 40, 5)

    def refused(state):
        arr = api.init_jobs([state])
        rc = api.lib().cms_init_two_view(ini.h, ctx.h, 1, arr)
        r = api.init_results(arr, [state])[0]
        untouched = (r["status"] == -7 and r["best_iteration"] == -7 and r["winner"] == -7 and (r["p3d"] == 7.0).all() and (r["triangulated"] == 9).all())
        return rc, untouched
    assert refused(api.init_job_state(ic.trim(pr, 7), ic.draws(1, 8, 5))) == (-1, True)             # N = 7
    e = d.copy(); e[2, 0] = 40
    assert refused(api.init_job_state(pr, e)) == (-1, True)
    e = d.copy(); e[4, 7] = 33
    assert refused(api.init_job_state(pr, e)) == (-1, True)
    m = pr["matches12"].copy(); m[np.flatnonzero(m >= 0)[5]] = len(pr["keys2"])
    assert refused(api.init_job_state(dict(pr, matches12=m), d)) == (-1, True)                      # a match index >= n2
    big = ic.problem(33, N=5000)
    assert refused(api.init_job_state(big, ic.draws(34, 5000, 2))) == (-1, True)                    # above the handle's matches
    assert refused(api.init_job_state(pr, ic.draws(35, 40, 5000))) == (-1, True)                    # above the handle's hypotheses
    # the handle is usable afterwards
    want, got = both(ctx, ini, cosfov, lambda: [api.init_job_state(pr, d)])
    same(want, got)


def test_handle_reuse(ctx, ini, cosfov):
    """A large call, a small one, the large one again: the blocks are grown once and reused, and the results are those of a fresh handle"""
    large = sized_states(60, 400)
    small = lambda: [api.init_job_state(ic.problem(41, N=30), ic.draws(42, 30, 9))]
    fresh = api.TwoViewInitializer(16, 4096, 8192, 4096)
    try:
        want_l = fresh.run(ctx, large())
    finally:
        fresh.close()
    fresh = api.TwoViewInitializer(16, 4096, 8192, 4096)
    try:
        want_s = fresh.run(ctx, small())
    finally:
        fresh.close()
    same(want_l, ini.run(ctx, large()))
    same(want_s, ini.run(ctx, small()))
    same(want_l, ini.run(ctx, large()))


def test_two_view_frames_equals_two_view(ctx, ini, cosfov):
    """cms_init_two_view_frames (key point and key ray of frame 2 taken on the device from the row the extractor left) against cms_init_two_view and the
    host core on the same data fetched to the host: two jobs on one row with different match lists"""
    ctx.set_mask(synth.cubemap_valid_mask(CAMD))
    k, _ = ctx.remap_extract(synth.texture(CAMD["Ih"], CAMD["Iw"], 3))
    rays = ctx.fetch_rays(0)
    n = len(k)
    assert n > 200 and len(rays) == n
    keys2 = np.stack([k["x"], k["y"]], 1).astype(np.float32)

    def states(frames):
        out = []
        for j, N in enumerate((150, 77)):
            r = np.random.default_rng(50 + j)
            idx = np.sort(r.choice(np.flatnonzero(rays[:, 2] > 0.3), N, replace=False))
            R, t = ic.pose(r)
            X2 = rays[idx].astype(np.float64) * r.uniform(2.0, 8.0, (N, 1))
            X1 = (X2 - t) @ R                                             # X2 = R X1 + t
            f1, u1, v1 = synth.rays_to_cubemap(F, X1)
            n1 = N + 11
            keys1 = ic.canvas_pixels(r, n1, F); at1 = np.sort(r.choice(n1, N, replace=False))
            good = f1 >= 0
            keys1[at1[good]] = np.stack([u1, v1], 1)[good]
            keys1 = keys1.astype(np.float32)
            m = np.full(n1, -1, np.int32); m[at1] = idx
            pr = dict(keys1=keys1, rays1=ic.unit_rays(F, keys1), keys2=keys2, rays2=rays, matches12=m)
            if frames:
                pr.update(keys2=np.zeros((1, 2), np.float32), rays2=np.zeros((1, 3), np.float32), n2=n)
            out.append(api.init_job_state(pr, ic.draws(60 + j, N, 50), b=0))
        return out
    rc, want = hl.two_view_host(F, cosfov, states(False))
    assert rc == 0 and want[0]["status"] == 1
    same(want, ini.run(ctx, states(False)))
    same(want, ini.run_frames(ctx, states(True)))
    # refused before anything is enqueued: a match at the row's count, a row beyond the batch
    bad = states(True); bad[0]["matches12"][np.flatnonzero(bad[0]["matches12"] >= 0)[2]] = n
    assert api.lib().cms_init_two_view_frames(ini.h, ctx.h, 2, api.init_jobs(bad)) == -1
    bad = states(True); bad[1]["b"] = 1
    assert api.lib().cms_init_two_view_frames(ini.h, ctx.h, 2, api.init_jobs(bad)) == -1


def test_mirror_class_on_the_device():
    """class Initializer (cubemap_hot_path.h) with its default engine, the device, against the same class over the host build of the core"""
    for seed, kw in ((3, dict(N=120)), (0, dict(N=200, noise=1.0, outliers=0.3)), (3, dict(N=120, baseline=0.0))):
        pr = ic.problem(seed, **kw)
        d = ic.draws(50 if seed == 0 else 5, pr["N"], 200)
        a = hl.mirror(1, CAMD, pr, 1.0, 200, d)
        b = hl.mirror(0, CAMD, pr, 1.0, 200, d)
        assert a["found"] == (0 if "baseline" in kw else 1)
        assert api.init_first_difference([a], [b]) is None, api.init_first_difference([a], [b])


E2E_GAP = 12      # frames 0 and 12 of synth.room_pose's loop: the smallest of the gaps 3, 5, 8, 12 at which the CPU chain below initialises (104 matches, 91 good)


def test_end_to_end_from_two_rendered_frames(ini):
    """Two rendered frames through device extraction (the 3 x nFeatures initialisation extractor), cms_search_for_initialization and
    cms_init_two_view_frames, against the CPU chain: oracle extraction, orc_search_for_initialization, host core -- bit for bit, and initialised"""
    import orc
    Fe, nf = 550, 6000
    camd = synth.camera("lafida", Fe)
    ocam = orc.make_camera(camd)
    scene = synth.room_scene(0xC0FFEE)
    mask = synth.cubemap_valid_mask(camd)
    frames = np.stack([synth.render_fisheye(camd, scene, *synth.room_pose(i, 300)) for i in (0, E2E_GAP)])
    # the CPU chain
    m1, m2 = orc.build_lut(ocam)
    cpu = []
    for f in frames:
        k, d = orc.Orb(nfeatures=nf).extract(ocam, orc.fisheye_to_cubemap(ocam, m1, m2, f), mask)
        cpu.append((k, d, orc.keyframe_rays(ocam, k["x"], k["y"])))
    (k1, d1, r1), (k2, d2, r2) = cpu
    prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
    want_m, want_n = orc.search_for_initialization(ocam, k1, d1, k2, d2, prev, 100, 0.9, True)
    assert want_n >= 100                                          # Tracking.cpp:432
    draws = ic.draws(77, want_n, 200)
    keys = lambda k: np.stack([k["x"], k["y"]], 1).astype(np.float32)
    rc, want = hl.two_view_host(Fe, hl.cos_fov(camd), [api.init_job_state(dict(keys1=keys(k1), rays1=r1, keys2=keys(k2), rays2=r2, matches12=want_m), draws)])
    assert rc == 0 and want[0]["status"] == 1 and want[0]["triangulated"].sum() >= 50
    # the device chain: frame 2 never leaves the device between extraction and the initializer
    c = api.Context(camd, nfeatures=nf, max_batch=2)
    try:
        c.set_mask(mask)
        c.upload(frames); c.process(2, True); c.sync()
        g1, gd1 = c.fetch(0)
        gr1 = c.fetch_rays(0)
        c.area_grid(2)
        prev = np.stack([g1["x"], g1["y"]], 1).astype(np.float32)
        got_m, got_n = c.search_for_initialization(1, g1, gd1, prev, 100, 0.9, True)
        assert got_n == want_n and np.array_equal(got_m, want_m)
        st = api.init_job_state(dict(keys1=keys(g1), rays1=gr1, keys2=np.zeros((1, 2), np.float32), rays2=np.zeros((1, 3), np.float32), matches12=got_m, n2=len(k2)),
                                draws, b=1)
        got = ini.run_frames(c, [st])
    finally:
        c.close()
    same(want, got)
