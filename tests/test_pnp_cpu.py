"""PnPsolver without a GPU: the shared core (cubemapslam_amd/csrc/cms_pnp_core.h) as the host build runs it (libcubemapslam_host.so), pinned from
outside stage by stage, by SVD-independent properties and by the noise-free n-point solve; the loop of PnPsolver::iterate on hand-made problems;
cms_pnp_ransac_parameters; the ABI.  The result of a four-point EPnP is defined by the SVD (DESIGN.md "PnPsolver"), so no restatement with another
SVD is compared with whole hypotheses."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import npref_pnp as ref
import pnp_cases as pc
import pnp_hostlib as hl
from cubemapslam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = pc.F


def literal_parameters(N, prob, min_inl, max_it, min_set, eps):
    eps = np.float32(eps)
    n_min = int(np.float32(N) * eps)
    n_min = max(n_min, min_inl, min_set)
    if eps < np.float32(n_min) / np.float32(N):
        eps = np.float32(n_min) / np.float32(N)
    its = 1 if n_min == N else math.ceil(math.log(1 - prob) / math.log(1 - math.pow(float(eps), 3)))
    return n_min, max(1, min(its, max_it))


def test_ransac_parameters():
    assert api.ransac_parameters(20, 0.99, 10, 300, 4, 0.5)[:2] == (10, 35)
    want = literal_parameters(15, 0.99, 10, 300, 4, 0.5)
    mi, it, eps = api.ransac_parameters(15, 0.99, 10, 300, 4, 0.5)
    assert (mi, it) == want and mi == 10 and eps == float(np.float32(10) / np.float32(15))
    assert api.ransac_parameters(4, 0.99, 4, 300, 4, 0.5)[:2] == (4, 1)
    assert api.ransac_parameters(200, 0.99, 10, 300, 4, 0.1)[:2] == (20, 300)
    assert api.ransac_parameters(200, 0.99, 10, 300, 4, 0.1)[:2] == literal_parameters(200, 0.99, 10, 300, 4, 0.1)
    # N < minSet: min_inliers = minSet > N (iterate() then says bNoMore), epsilon > 1, log of a negative number: one iteration
    assert api.ransac_parameters(3, 0.99, 2, 300, 4, 0.5)[:2] == (4, 1)
    assert api.ransac_parameters(60)[:2] == literal_parameters(60, 0.99, 8, 300, 4, 0.4)


@pytest.fixture(scope="module")
def solves():
    """200 solves of the core with every stage: 100 four-point, 50 eight-point, 50 forty-point (noise 0.5 px, 20 % outliers among the points)"""
    out = []
    for k in range(200):
        n = 4 if k < 100 else (8 if k < 150 else 40)
        pr = pc.problem(1000 + k, N=60, outliers=0.2, noise=0.5)
        st = api.pnp_job_state(pr, 1, [])
        idx = np.random.default_rng(k).choice(60, n, replace=False)
        out.append(hl.compute_pose(F, st, idx))
    return out


def _svd_residuals(A, w, Vt, AV, sym):
    s0 = max(w[0], 1e-300)
    r = dict(orth=np.abs(Vt @ Vt.T - np.eye(len(w))).max(), desc=float(np.max(np.diff(w).clip(min=0))) / s0)
    if sym:
        r["eig"] = max(np.linalg.norm(A @ Vt[i] - w[i] * Vt[i]) for i in range(len(w))) / s0
    else:
        r["eig"] = max(abs(np.linalg.norm(A @ Vt[i]) - w[i]) for i in range(len(w))) / s0
    r["av"] = max(np.linalg.norm(A @ Vt[i] - AV[i]) for i in range(len(w))) / s0
    return r


def test_svd_properties(solves):
    """Orthonormal rows, A v = d v (|A v| = d for the general 3 x 3), descending d, null space of a four-point MtM: within 100 x what numpy's LAPACK
    SVD leaves on the same matrices (relative to the largest singular value)"""
    worst = {}
    for s in solves:
        n = len(s["pws"])
        M = ref.build_M(s["alphas"], s["bearings"])
        ccs = sum(s["betas"][0][i] * s["ut"][11 - i].reshape(4, 3) for i in range(4))
        pcs = s["alphas"] @ ccs
        mats = [("mtm", M.T @ M, True), ("pca", ref.pca(s["pws"]), True), ("abt", (pcs - pcs.mean(0)).T @ (s["pws"] - s["pws"].mean(0)), False)]
        for name, A, sym in mats:
            if not np.isfinite(A).all():
                continue
            AV, w, Vt = hl.jacobi(A)
            U, wl, Vl = np.linalg.svd(A)
            for tag, r in (("core", _svd_residuals(A, w, Vt, AV, sym)), ("lapack", _svd_residuals(A, wl, Vl, (U * wl).T, sym))):
                for k, v in r.items():
                    worst[(name, k, tag)] = max(worst.get((name, k, tag), 0.0), v)
            if name == "mtm" and n == 4:
                worst[("mtm", "null4", "core")] = max(worst.get(("mtm", "null4", "core"), 0.0), w[8:].max() / w[0])
                worst[("mtm", "null4", "lapack")] = max(worst.get(("mtm", "null4", "lapack"), 0.0), wl[8:].max() / wl[0])
            assert np.abs(w - wl).max() <= 1e-9 * wl[0]
    for (name, k, tag), v in sorted(worst.items()):
        print("svd %-4s %-6s %-7s %.3e" % (name, k, tag, v))
    for (name, k, tag), v in worst.items():
        if tag == "core":
            assert v <= 100 * max(worst[(name, k, "lapack")], np.finfo(np.float64).eps), (name, k, v, worst[(name, k, "lapack")])


def test_stage_fed_by_stage(solves):
    """The restatement is fed the core's own uct / dc and ut; every later stage then agrees to 1e-9 (scenes of unit scale).  A solve is left out only
    when one of its least-squares matrices (numpy's cond on the core's own A) reaches 1e6; at most 2 % may be."""
    tol, skipped, worst = 1e-9, 0, 0.0
    for s in solves:
        pws, us, ut = s["pws"], s["us"], s["ut"]
        cws = ref.control_points(pws, s["dc"], s["uct"])
        assert np.abs(cws - s["cws"]).max() <= tol
        al = ref.barycentric(pws, s["cws"])
        assert np.abs(al - s["alphas"]).max() <= tol
        assert np.abs(s["alphas"] @ s["cws"] - pws).max() <= tol and np.abs(s["alphas"].sum(1) - 1).max() <= tol
        L = ref.L_6x10(ut); rh = ref.rho(s["cws"])
        assert np.abs(L - s["L"]).max() <= tol and np.abs(rh - s["rho"]).max() <= tol
        conds, errs, reps = [], [], []
        for which in (1, 2, 3):
            b0, A = ref.betas_approx(which, s["L"], s["rho"])
            conds.append(np.linalg.cond(A))
            errs.append(np.abs(b0 - s["betas0"][which - 1]).max())
            be, c = ref.gauss_newton(s["L"], s["rho"], s["betas0"][which - 1])
            conds.append(c)
            errs.append(np.abs(be - s["betas"][which - 1]).max())
            R, t, e = ref.R_and_t(F, pws, us, s["alphas"], ut, s["betas"][which - 1])
            errs += [np.abs(R - s["Rs"][which - 1]).max(), np.abs(t - s["ts"][which - 1]).max(), abs(e - s["rep"][which - 1])]
            reps.append(s["rep"][which - 1])
        if not np.isfinite(conds).all() or max(conds) >= 1e6:
            skipped += 1
            continue
        assert max(errs) <= tol, (errs, conds)
        worst = max(worst, max(errs))
        n = 1
        if reps[1] < reps[0]:
            n = 2
        if reps[2] < reps[n - 1]:
            n = 3
        assert s["chosen"] == n and np.array_equal(s["R"], s["Rs"][n - 1]) and np.array_equal(s["t"], s["ts"][n - 1]) and s["rep_error"] == reps[n - 1]
    print("stage by stage: worst difference %.3e over %d solves, %d left out for cond >= 1e6" % (worst, len(solves) - skipped, skipped))
    assert skipped <= 0.02 * len(solves), skipped


def test_noise_free_n_point_solve():
    """n = 6, 12, 40 exact correspondences (float32 inputs): the core against the LAPACK restatement and against the truth, within 4 x the
    disagreement of the restatement's own LAPACK and plain-Jacobi variants on the same cases"""
    rows = []
    for n in (6, 12, 40):
        for seed in range(7):
            pr = pc.problem(200 + 10 * n + seed, N=n, outliers=0.0, front_first=True)
            s = hl.compute_pose(F, api.pnp_job_state(pr, 1, []), np.arange(n))
            Rl, tl, _ = ref.compute_pose(F, s["pws"], s["us"], s["bearings"])
            Rj, tj, _ = ref.compute_pose(F, s["pws"], s["us"], s["bearings"], svd=ref.svd_jacobi)
            rows.append((np.abs(Rl - Rj).max(), np.abs(tl - tj).max(), np.abs(s["R"] - Rl).max(), np.abs(s["t"] - tl).max(), np.abs(s["R"] - pr["R"]).max(),
                         np.abs(s["t"] - pr["t"]).max(), np.abs(Rl - pr["R"]).max(), np.abs(tl - pr["t"]).max()))
    m = np.array(rows).max(0)
    print("noise-free: restatement LAPACK vs Jacobi dR %.2e dt %.2e | core vs LAPACK dR %.2e dt %.2e | core vs truth dR %.2e dt %.2e | LAPACK vs truth dR %.2e dt %.2e" % tuple(m))
    assert m[2] <= 4 * m[0] and m[3] <= 4 * m[1]
    assert m[4] <= 4 * max(m[0], m[6]) and m[5] <= 4 * max(m[1], m[7])


def test_check_inliers_bit_for_bit():
    rng = np.random.default_rng(3)
    total = quirk = nobranch = 0
    for k in range(12):
        pr = pc.problem(300 + k, N=400, outliers=0.3, noise=1.5)
        R, t = pr["R"], pr["t"]
        if k % 3 == 1:
            R, t = pc.random_pose(rng)
        p3d = pr["p3d"].copy()
        p3d[:5] = 0; p3d[0] = (-R.T @ t).astype(np.float32)          # the camera centre and the origin: next to no branch / no branch
        me = (pr["sigma2"] * np.float32(5.991)).astype(np.float32)
        want = ref.check_inliers(F, R, t, p3d, pr["p2d"], me)
        got = hl.check_inliers(F, R, t, p3d, pr["p2d"], me)
        assert np.array_equal(got, want), k
        total += len(want)
    # no branch at all: the camera-frame point is exactly zero -> ue = ve = -1; a pixel near (-1, -1) is then an "inlier"
    I = np.eye(3); z = np.zeros(3)
    p3d = np.zeros((4, 3), np.float32); p2d = np.array([[-1, -1], [0, 0], [-1, 1.4], [300, 300]], np.float32); me = np.full(4, 5.991, np.float32)
    want = ref.check_inliers(F, I, z, p3d, p2d, me)
    assert list(want) == [True, True, True, False] and np.array_equal(hl.check_inliers(F, I, z, p3d, p2d, me), want)
    nobranch += 4
    # in a branch but outside the face (the ratio is exactly 1: u = F): UNKNOWN, yet ue, ve hold the in-face values, without the face's offset
    p3d = np.array([[1, 0.5, 1], [2, -2, 2], [1, 1, 1]], np.float32)
    face, ue, ve = ref.rays_to_cubemap(F, p3d[:, 0], p3d[:, 1], p3d[:, 2])
    assert list(face) == [-1, -1, -1] and list(ue) == [F, F, F] and ve[0] == np.float32(0.75 * F)
    p2d = np.stack([ue, ve], 1) + np.array([[1, 1], [0, 0], [3, 0]], np.float32); me = np.full(3, 5.991, np.float32)
    want = ref.check_inliers(F, I, z, p3d, p2d, me)
    assert list(want) == [True, True, False] and np.array_equal(hl.check_inliers(F, I, z, p3d, p2d, me), want)
    quirk += 3
    # error2 exactly at the bound: 3^2 + 4^2 = 25 against 25 (strict <) and against the next float
    p3d = np.array([[0, 0, 2], [0, 0, 2]], np.float32); c = np.float32(F / 2 + F)
    p2d = np.array([[c + 3, c + 4], [c + 3, c + 4]], np.float32); me = np.array([25, np.nextafter(np.float32(25), np.float32(26))], np.float32)
    want = ref.check_inliers(F, I, z, p3d, p2d, me)
    assert list(want) == [False, True] and np.array_equal(hl.check_inliers(F, I, z, p3d, p2d, me), want)
    assert total >= 4000


# ---- the loop -------------------------------------------------------------------------------------------------------------------------------
N_IN, N_OUT = 12, 8


@pytest.fixture(scope="module")
def exact():
    pr = pc.exact_problem(5, N_IN, N_OUT)
    # quadruples of inliers that recover all inliers, searched on the host build (not every exact quadruple does: the basis the SVD picks inside
    # MtM's null space decides, and solve_for_sign wants the first point in front)
    rng = np.random.default_rng(0)
    found = []
    for _ in range(200):
        q = [int(v) for v in rng.choice(N_IN, 4, replace=False)]
        if pr["zc"][q[0]] > 0.5 and q not in found and run(pr, [q], 1, N_IN, 1)[1]["best_inliers"] == N_IN:
            found.append(q)
        if len(found) == 2:
            break
    assert len(found) == 2
    return pr, found


def run(pr, sets_or_draws, n_iterations, min_inliers, max_its, raw=False, **state):
    q = dict(pr, min_inliers=min_inliers, max_its=max_its, **state)
    if not raw:      # the caller draws for every iteration the call may need: the listed quadruples, then ones with two outliers
        H = max(max_its - state.get("iterations", 0), n_iterations)
        sets_or_draws = list(sets_or_draws) + [[N_IN, N_IN + 1, 0, 1]] * max(0, H - len(sets_or_draws))
    d = np.asarray(sets_or_draws, np.int32) if raw else pc.draws_for(sets_or_draws, len(pr["p3d"]))
    st = api.pnp_job_state(q, n_iterations, d)
    rc, res = hl.iterate_host(F, [st])
    return rc, (res[0] if res else None)


def good(found, k=0):
    return found[k]


def test_swap_and_pop():
    N = 20
    rows = [[0, 0, 0, 0], [19, 18, 17, 16], [5, 5, 17, 5], [18, 0, 17, 0], [19, 0, 0, 16], [3, 18, 3, 3]]
    rng = np.random.default_rng(0)
    rows += [[int(rng.integers(0, N - k)) for k in range(4)] for _ in range(300)]
    for N_, rs in ((N, rows), (4, [[3, 2, 1, 0], [0, 0, 0, 0], [3, 0, 1, 0]]), (5, [[4, 3, 2, 1], [0, 3, 0, 1]])):
        for r in rs:
            idx = np.zeros(4, np.int32)
            hl.H().hm_pnp_resolve_draws(N_, hl.p(np.array(r, np.int32)), hl.p(idx))
            assert list(idx) == pc.swap_and_pop(N_, r) and len(set(idx)) == 4, (N_, r)


def test_loop_accepts_on_more_than_min_inliers(exact):
    pr, front = exact
    bad = [N_IN, 0, 1, 2]
    rc, r = run(pr, [bad, good(front), good(front, 1)], 5, N_IN - 1, 13)
    assert rc == 0 and r["status"] == 1 and r["no_more"] == 0 and r["iterations"] == 2 and r["iterations_run"] == 2 and r["n_inliers"] == N_IN
    assert list(r["inliers"]) == [1] * N_IN + [0] * N_OUT and r["best_inliers"] == N_IN and np.array_equal(r["best_mask"], r["inliers"])
    T = r["Tcw"]
    assert np.abs(T[:9].reshape(3, 3) - pr["R"]).max() < 1e-5 and np.abs(T[9:] - pr["t"]).max() < 1e-4
    # exactly min_inliers: the hypothesis qualifies (>=), Refine is not accepted (>): the loop runs on to max_its -- `||`: 5 asked, 13 run
    sets = [good(front)] + [bad] * 12
    rc, r = run(pr, sets, 5, N_IN, 13)
    assert rc == 0 and r["status"] == 2 and r["no_more"] == 1 and r["iterations"] == 13 and r["iterations_run"] == 13 and r["n_inliers"] == N_IN
    assert list(r["inliers"]) == [1] * N_IN + [0] * N_OUT and np.array_equal(r["Tcw"], r["best_Tcw"])
    # ... and the other side of `||`: max_its reached before the call, 5 asked, 5 run
    rc, r = run(pr, [bad] * 5, 5, N_IN, 3)
    assert r["iterations_run"] == 5 and r["iterations"] == 5 and r["no_more"] == 1 and r["status"] == 0


def test_loop_best_only_on_more(exact):
    pr, front = exact
    a, b = good(front), good(front, 1)
    _, ra = run(pr, [a], 1, N_IN, 1)
    _, rb = run(pr, [b], 1, N_IN, 1)
    assert ra["status"] == 2 and rb["status"] == 2 and ra["best_inliers"] == rb["best_inliers"] == N_IN
    assert not np.array_equal(ra["best_Tcw"], rb["best_Tcw"])          # two four-point solves: the same pose, other bits
    _, rab = run(pr, [a, b], 2, N_IN, 2)
    _, rba = run(pr, [b, a], 2, N_IN, 2)
    assert np.array_equal(rab["best_Tcw"], ra["best_Tcw"]) and np.array_equal(rba["best_Tcw"], rb["best_Tcw"])


def test_loop_refines_the_best_mask(exact):
    """A best carried in with more (but wrong) inliers: a later, weaker hypothesis qualifies, does not become the best, and Refine runs on the
    carried mask -- and fails; refining the hypothesis's own mask would have been accepted"""
    pr, front = exact
    mask = np.zeros(N_IN + N_OUT, np.uint8); mask[:6] = 1; mask[N_IN:N_IN + 7] = 1
    T = np.arange(12, dtype=np.float32)
    rc, r = run(pr, [good(front)], 1, 10, 1, best_inliers=13, best_mask=mask, best_Tcw=T)
    assert rc == 0 and r["status"] == 2 and r["best_inliers"] == 13 and np.array_equal(r["best_mask"], mask) and np.array_equal(r["Tcw"], T) and r["n_inliers"] == 13
    rc, r = run(pr, [good(front)], 1, 10, 1)
    assert r["status"] == 1 and r["n_inliers"] == N_IN


def test_loop_exhaustion_and_small_N(exact):
    pr, front = exact
    bad = [N_IN, N_IN + 1, 0, 1]
    rc, r = run(pr, [bad] * 4, 4, 10, 4)
    assert rc == 0 and r["status"] == 0 and r["no_more"] == 1 and r["n_inliers"] == 0 and r["best_inliers"] == 0 and not r["inliers"].any() and not r["Tcw"].any()
    rc, r = run(pr, [bad] * 2, 2, 10, 4)
    assert r["status"] == 0 and r["no_more"] == 1 and r["iterations"] == 4 and r["iterations_run"] == 4
    rc, r = run(pr, [], 5, N_IN + N_OUT + 1, 13, iterations=3)
    assert rc == 0 and r["no_more"] == 1 and r["status"] == 0 and r["iterations"] == 3 and r["iterations_run"] == 0


def test_two_calls_equal_one(exact):
    pr, front = exact
    d = pc.draws(11, N_IN + N_OUT, 13)
    d[4] = pc.draws_for([good(front)], N_IN + N_OUT)[0]; d[9] = pc.draws_for([good(front, 1)], N_IN + N_OUT)[0]
    _, one = run(pr, d, 5, N_IN, 13, raw=True)
    _, r1 = run(pr, d[:6], 6, N_IN, 6, raw=True)
    assert r1["iterations"] == 6 and r1["best_inliers"] == N_IN
    _, r2 = run(pr, d[6:], 1, N_IN, 13, raw=True, iterations=r1["iterations"], best_inliers=r1["best_inliers"], best_mask=r1["best_mask"], best_Tcw=r1["best_Tcw"])
    assert r2["iterations_run"] == 7
    for k in ("status", "no_more", "n_inliers", "iterations", "best_inliers"):
        assert one[k] == r2[k], k
    for k in ("Tcw", "best_Tcw", "inliers", "best_mask"):
        assert np.array_equal(one[k], r2[k]), k


def test_error_codes(exact):
    pr, front = exact
    N = N_IN + N_OUT
    d = pc.draws(1, N, 5)
    for k, v in ((0, N), (1, N - 1), (3, N - 3), (2, -1)):
        e = d.copy(); e[4, k] = v
        assert run(pr, e, 5, 10, 5, raw=True)[0] == -1
    assert run(pr, d[:4], 5, 10, 5, raw=True)[0] == -1                      # fewer than 4 * H draws
    assert run(pr, d, 5, 10, 5, raw=True, best_inliers=3)[0] == -1          # best_mask (empty) against best_inliers
    st = api.pnp_job_state(dict(pr, min_inliers=10, max_its=5), 5, d, min_set=5)
    assert hl.iterate_host(F, [st])[0] == -3
    assert run(pr, d, 5, 10, 5, raw=True)[0] == 0


def test_exports_and_job_layout(tmp_path):
    L = api.lib()
    for name in ("cms_pnp_ransac_parameters", "cms_pnp_create", "cms_pnp_destroy", "cms_pnp_iterate"):
        assert hasattr(L, name), name
    assert hasattr(hl.H(), "hm_pnp_iterate_host")
    fields = [f[0] for f in api.PnpJob._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cubemapslam_hip.h"\nint main(void) {\n  printf("%zu", sizeof(cms_pnp_job));\n' +
                   "".join('  printf(" %%zu", offsetof(cms_pnp_job, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(api.PnpJob) and out[1:] == [getattr(api.PnpJob, f).offset for f in fields]


def test_core_header_alone_under_gpp(tmp_path):
    """cms_pnp_core.h compiled on its own by g++ (tests/emu/pnp_core_emu.cpp) gives the host library's bits, stage for stage"""
    so = tmp_path / "pnp_core_emu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-fPIC", "-shared", "-I", os.path.join(ROOT, "cubemapslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "pnp_core_emu.cpp"), "-o", str(so)])
    E = C.CDLL(str(so))
    E.emu_compute_pose.restype = C.c_double
    E.emu_compute_pose.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 8
    assert E.emu_stages_size() == C.sizeof(hl.Stages)
    for n, seed in ((4, 1), (4, 2), (9, 3), (33, 4)):
        pr = pc.problem(seed, N=40, outliers=0.2, noise=0.7)
        s = hl.compute_pose(F, api.pnp_job_state(pr, 1, []), np.arange(n) + 3)
        st = hl.Stages(); ut = np.zeros((12, 12)); al = np.zeros((n, 4)); R = np.zeros((3, 3)); t = np.zeros(3)
        pws, us, be = (np.ascontiguousarray(s[k]) for k in ("pws", "us", "bearings"))
        e = E.emu_compute_pose(n, F, hl.p(pws), hl.p(us), hl.p(be), C.byref(st), hl.p(ut), hl.p(al), hl.p(R), hl.p(t))
        assert e == s["rep_error"] and np.array_equal(R, s["R"]) and np.array_equal(t, s["t"]) and np.array_equal(ut, s["ut"]) and np.array_equal(al, s["alphas"])
        assert np.array_equal(np.array(st.betas[:]).reshape(3, 4), s["betas"]) and st.chosen == s["chosen"]


def test_golden_cases_exactly():
    """tests/golden/pnp_v1.npz: inputs, draws and the host build's outputs of six jobs, compared exactly -- a change of the order of the core's
    operations has to regenerate the file (tests/golden/make_pnp_golden.py) and say so"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_pnp_golden", os.path.join(ROOT, "tests", "golden", "make_pnp_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    z = np.load(os.path.join(ROOT, "tests", "golden", "pnp_v1.npz"))
    n = int(z["count"])
    assert n == 6
    st = [G.state_from(z, j) for j in range(n)]
    rc, res = hl.iterate_host(int(z["F"]), st)
    assert rc == 0
    for j, r in enumerate(res):
        for k in G.OUT_SCALARS:
            assert r[k] == int(z["out%d_%s" % (j, k)]), (j, k)
        for k in G.OUT_KEYS:
            assert np.array_equal(r[k].view(np.uint8), z["out%d_%s" % (j, k)].view(np.uint8)), (j, k)
    assert sorted(set(int(z["out%d_status" % j]) for j in range(n))) == [0, 1, 2]


def test_first_point_behind_the_front_plane_comes_out_mirrored():
    """solve_for_sign (:647-660) looks at the FIRST point's camera z only.  Exact correspondences whose first point has z < 0: the solve puts that point
    in front, estimate_R_and_t fits a proper rotation to the negated camera points (far from the true pose, reprojection error of hundreds of pixels), and it is still the solve the independent LAPACK restatement makes -- the quirk is kept, not an accident"""
    rows, used = [], 0
    for seed in range(400, 440):
        pr = pc.problem(seed, N=12, outliers=0.0)
        if not pr["zc"][0] < -0.5:
            continue
        used += 1
        s = hl.compute_pose(F, api.pnp_job_state(pr, 1, []), np.arange(12))
        assert (pr["R"] @ s["pws"][0] + pr["t"])[2] < 0 and abs(np.linalg.det(s["R"]) - 1) < 1e-9      # a proper rotation fitted to the negated points
        assert max(np.abs(s["R"] - pr["R"]).max(), np.abs(s["t"] - pr["t"]).max()) > 0.1 and s["rep_error"] > 10.0
        Rl, tl, _ = ref.compute_pose(F, s["pws"], s["us"], s["bearings"])
        Rj, tj, _ = ref.compute_pose(F, s["pws"], s["us"], s["bearings"], svd=ref.svd_jacobi)
        rows.append((np.abs(Rl - Rj).max(), np.abs(tl - tj).max(), np.abs(s["R"] - Rl).max(), np.abs(s["t"] - tl).max()))
        if used == 6:
            break
    m = np.array(rows).max(0)
    print("mirrored: restatement LAPACK vs Jacobi dR %.2e dt %.2e | core vs LAPACK dR %.2e dt %.2e over %d cases" % (tuple(m) + (used,)))
    assert used == 6 and m[2] <= 4 * m[0] and m[3] <= 4 * m[1]
