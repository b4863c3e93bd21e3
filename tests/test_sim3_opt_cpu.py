"""OptimizeSim3 on the CPU: the host build of cubemapslam_amd/csrc/cms_sim3_opt_core.h (libcubemapslam_host.so: hm_sim3_optimize_host and its stage
probes) against the numpy restatement of the reference's and g2o's text (npref_sim3_opt), stage by stage and over whole runs, bit for bit.

The restatement takes exp / sin / cos as callables; for the bit-for-bit comparisons it gets the core's own (through the probes), because libm's
differ from any fixed-order polynomial in the last place and a Sim3 that differs in the last place flips float residuals.  How far the core's
exp / sin / cos are from libm's is measured here and printed (tools/prof_sim3_opt.py writes the same figures to profiles/sim3_opt_parity.md); it is
not a bar, the core is the definition of record.

Bars that are not bit-equalities:
  analytic Jacobian   against central differences (delta = 1e-6) of the restatement's error with a DOUBLE projection: max |dJ| <= 1e-5 * max |J| per
                      edge.  Round-off of the difference is about 2.2e-16 * 550 / 2e-6 = 6e-8 against |J| >= 30, its truncation delta^2 * J''' / 6
                      is below that, a wrong term is O(1) relative
  non-zero share      of the as-written Jacobian, on the restatement only: a 1e-9 step moves a projected coordinate by ~1e-9 * |J| ~ 5e-8 pixel, a
                      float near 275 is spaced 3e-5: a coordinate crosses a rounding boundary in about 2 * 5e-8 / 3e-5 = 0.3 % of the cases, and either
                      of the 2 evaluations may.  Asserted below 5 %, far from the 100 % of a working derivative"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import npref_sim3_opt as ref
import sim3_opt_cases as sc
import sim3_opt_hostlib as hl
from cubemapslam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = sc.F
f64 = np.float64


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f64)).tobytes()


def ulps(a, b):
    """distance in units of the last place between two finite doubles of the same sign region"""
    ia = np.array([a], f64).view(np.int64)[0]; ib = np.array([b], f64).view(np.int64)[0]
    return abs(int(ia) - int(ib))


def start_of(case):
    return ref.sim3_from_Rts(np.asarray(case["R12"], f64).reshape(3, 3), case["t12"], case["s12"])


@pytest.fixture(scope="module")
def case300():
    return sc.case(11, N=300, outliers=0.2, fix_scale=0)


# ---- deterministic exp / sin / cos
def det_libm_distances():
    """max ulp distance of the core's exp / sin / cos from libm's over the arguments that occur: |theta| <= pi, |sigma| <= 1, the 1e-9 neighbourhood"""
    rng = np.random.default_rng(3)
    thetas = np.concatenate([rng.uniform(1e-5, np.pi, 20000), np.geomspace(1e-5, np.pi, 2000), [np.pi, np.pi / 2, np.pi / 4, 1e-5, 3 * np.pi / 4]])
    sigmas = np.concatenate([rng.uniform(-1, 1, 20000), np.geomspace(1e-12, 1, 2000), -np.geomspace(1e-12, 1, 2000), [0.0, 1e-9, -1e-9, 1.0, -1.0, 1e-5, -1e-5]])
    d = dict(exp=0, sin=0, cos=0)
    for s in sigmas:
        d["exp"] = max(d["exp"], ulps(hl.det_exp(s), math.exp(s)))
    for t in thetas:
        sn, cs = hl.det_sincos(t)
        d["sin"] = max(d["sin"], ulps(sn, math.sin(t)))
        # cos near pi / 2 is tiny: its ulps measure the argument reduction, not the series; counted where |cos| >= 1e-3
        if abs(math.cos(t)) >= 1e-3:
            d["cos"] = max(d["cos"], ulps(cs, math.cos(t)))
    return d


def test_det_exp_sincos_against_libm():
    d = det_libm_distances()
    print("max ulp distance from libm: exp %(exp)d, sin %(sin)d, cos %(cos)d" % d)
    assert all(math.isfinite(v) for v in d.values())
    assert hl.det_exp(0.0) == 1.0 and hl.det_sincos(0.0) == (0.0, 1.0)
    assert math.isnan(hl.det_exp(float("nan"))) and all(math.isnan(v) for v in hl.det_sincos(float("nan")))
    # the 1e-5 branch boundaries of Sim3(update): the core and the restatement (with the core's functions) take the same branch on either side,
    # and libm's functions give finite values there as well
    eps = 0.00001
    for theta in (np.nextafter(eps, 0), eps, np.nextafter(eps, 1)):
        for sigma in (np.nextafter(eps, 0), eps, np.nextafter(eps, 1), -eps, 0.0):
            u = np.array([theta, 0, 0, 0.1, -0.2, 0.3, sigma])
            g = hl.sim3_exp(u); w = ref.sim3_exp(u, hl.FN); m = ref.sim3_exp(u)
            assert bits(np.concatenate([g[0], g[1], [g[2]]])) == bits(np.concatenate([w[0], w[1], [w[2]]])), (theta, sigma)
            assert np.isfinite(np.concatenate([m[0], m[1], [m[2]]])).all()


# ---- stage by stage
def test_exponential_and_quaternion_of_R():
    rng = np.random.default_rng(5)
    for k in range(200):
        u = rng.normal(size=7) * rng.choice([1e-9, 1e-6, 1e-3, 0.3, 1.0])
        if k % 5 == 0:
            u[6] = 0.0
        if k % 7 == 0:
            u[:3] = 0.0
        if k % 11 == 0:
            u[:3] *= np.pi / max(np.linalg.norm(u[:3]), 1e-300)      # |theta| = pi
        g = hl.sim3_exp(u); w = ref.sim3_exp(u, hl.FN)
        assert bits(g[0]) == bits(w[0]) and bits(g[1]) == bits(w[1]) and bits(g[2]) == bits(w[2]), (k, u)
    from cubemapslam_amd import synth
    for k in range(200):      # Quaterniond(R): all four branches (the trace and each of the three diagonal entries largest)
        R = synth._rot(rng.normal(size=3), rng.uniform(-np.pi, np.pi))
        assert bits(hl.R_to_quat(R)) == bits(ref.quat_from_R(R)), k
    branches = set()
    for k in range(200):
        R = synth._rot(rng.normal(size=3), rng.uniform(2.5, np.pi))
        branches.add(-1 if np.trace(R) > 0 else int(np.argmax(np.diag(R))))
    assert {0, 1, 2} <= branches


def test_oplus_and_inverse(case300):
    rng = np.random.default_rng(6)
    S = start_of(case300)
    for fix in (0, 1):
        u = rng.normal(size=7) * 0.01
        g, ug = hl.oplus(S, u, fix)
        uw = u.copy(); w = ref.oplus(S, uw, fix, hl.FN)
        assert all(bits(a) == bits(b) for a, b in zip(g, w)) and bits(ug) == bits(uw) and (uw[6] == 0) == bool(fix)
    gi = hl.inverse(S); wi = ref.sim3_inverse(S)
    assert all(bits(a) == bits(b) for a, b in zip(gi, wi))


@pytest.mark.parametrize("fix_scale", (0, 1))
def test_edge_error_and_as_written_jacobian(case300, fix_scale):
    """The float-narrowed error of both edges and g2o's numeric Jacobian, per correspondence, bit-equal; all five faces on both sides"""
    S = start_of(case300)
    P = ref.make_pairs(F, case300)
    assert set(P["face1"]) == {0, 1, 2, 3, 4} and set(P["face2"]) == {0, 1, 2, 3, 4}
    assert np.array_equal(P["face1"], case300["face1"]) and np.array_equal(P["face2"], case300["face2"])
    e12, e21 = ref.errors(F, P, S)
    J12, J21 = ref.numeric_jacobians(F, P, S, fix_scale, hl.FN)
    for k in range(0, 300, 3):
        g12, g21 = hl.edge_errors(F, S, case300, k)
        assert bits(g12) == bits(e12[k]) and bits(g21) == bits(e21[k]), k
        j12, j21 = hl.edge_jacobians(F, 0, fix_scale, S, case300, k)
        assert bits(j12) == bits(J12[k]) and bits(j21) == bits(J21[k]), k
    if fix_scale:      # every update is exp(0) = 1 exactly or below 1e-5: libm's functions give the same bits
        L12, L21 = ref.numeric_jacobians(F, P, S, fix_scale)
        assert bits(L12) == bits(J12) and bits(L21) == bits(J21)
        assert not J12[:, :, 6].any() and not J21[:, :, 6].any()


def test_solve7_and_slot_tree():
    rng = np.random.default_rng(7)
    for k in range(50):
        A = rng.normal(size=(9, 7)); H = A.T @ A; H = (H + H.T) / 2; b = rng.normal(size=7)
        if k % 10 == 0:
            H[:, 6] = 0; H[6, :] = 0      # fix_scale: an empty row and column, the pivot is lambda
        lam = 1e-5 * np.abs(np.diag(H)).max()
        ok_g, xg = hl.solve7(H, b, lam); ok_w, xw = ref.solve7(H, b, lam)
        assert ok_g == ok_w and ok_g and bits(xg) == bits(xw), k
    ok_g, xg = hl.solve7(np.zeros((7, 7)), np.ones(7), 0.0); ok_w, xw = ref.solve7(np.zeros((7, 7)), np.ones(7), 0.0)
    assert not ok_g and not ok_w
    for k in range(20):
        s = rng.normal(size=ref.SLOTS) * 10.0 ** rng.integers(-8, 8, ref.SLOTS)
        assert bits(hl.tree(s)) == bits(ref.tree(s)[0]), k
    # the tree is a sum (close to the exact one) and it is not the plain left-to-right sum: on slots of mixed magnitude the two differ in their bits
    differ = 0
    for k in range(20):
        s = rng.normal(size=ref.SLOTS) * 10.0 ** rng.integers(-8, 8, ref.SLOTS)
        t = hl.tree(s)
        assert t == pytest.approx(math.fsum(s), rel=1e-9)
        seq = 0.0
        for v in s:
            seq += float(v)
        differ += bits(t) != bits(seq)
    assert differ >= 10


# ---- whole runs
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("N", (0, 9, 10, 11, 64, 300))
def test_whole_run_equals_the_restatement(N, mode):
    for fix, outl in ((0, 0.3), (1, 0.3), (0, 0.0)):
        c = sc.case(100 + N + fix, N=N, outliers=outl, fix_scale=fix)
        rc, got = hl.optimize_host(F, [api.sim3_opt_job_state(c, sc.TH2, jacobian=mode)])
        assert rc == 0
        want = ref.optimize_sim3(F, c, sc.TH2, fix, mode, hl.FN)
        diff = api.sim3_opt_first_difference([want], got)
        assert diff is None, (fix, outl, diff)


# ---- the analytic Jacobian
@pytest.mark.parametrize("fix_scale", (0, 1))
def test_analytic_jacobian_against_central_differences(case300, fix_scale):
    S = start_of(case300)
    P = ref.make_pairs(F, case300)
    N12, N21 = ref.numeric_jacobians(F, P, S, fix_scale, delta=1e-6, narrow=False)
    worst = 0.0
    for k in range(300):
        j12, j21 = hl.edge_jacobians(F, 1, fix_scale, S, case300, k)
        for J, Nn in ((j12, N12[k]), (j21, N21[k])):
            assert np.abs(J).max() > 1.0
            rel = np.abs(J - Nn).max() / np.abs(J).max()
            worst = max(worst, rel)
            assert rel <= 1e-5, (k, rel)
        if fix_scale:
            assert not j12[:, 6].any() and not j21[:, 6].any()
        else:      # e12's scale column is Jpi(y) y = 0 up to rounding (the projection does not see the length of y); e21's is not
            assert j21[:, 6].any() and np.abs(j12[:, 6]).max() <= 1e-9 * np.abs(j12).max()
    print("analytic Jacobian against central differences: worst max|dJ| / max|J| = %.3g" % worst)
    # and the restatement's analytic Jacobian is the core's, bit for bit
    A12, A21 = ref.analytic_jacobians(F, P, S, fix_scale)
    for k in range(0, 300, 7):
        j12, j21 = hl.edge_jacobians(F, 1, fix_scale, S, case300, k)
        assert bits(j12) == bits(A12[k]) and bits(j21) == bits(A21[k])


def as_written_nonzero_share(case):
    S = start_of(case)
    P = ref.make_pairs(F, case)
    J12, J21 = ref.numeric_jacobians(F, P, S, False)
    A12, A21 = ref.analytic_jacobians(F, P, S, False)
    J = np.concatenate([J12.ravel(), J21.ravel()]); A = np.concatenate([A12.ravel(), A21.ravel()])
    nz = J != 0
    return float(nz.mean()), float(np.median(np.abs(J[nz]))) if nz.any() else 0.0, float(np.median(np.abs(A)))


def test_the_as_written_jacobian_is_almost_all_zeros(case300):
    """The finding, on the restatement alone (libm's functions, none of the product's code)"""
    share, med_nz, med_true = as_written_nonzero_share(case300)
    print("as-written Jacobian: %.2f %% of the entries non-zero, their median magnitude %.3g, median true magnitude %.3g" % (100 * share, med_nz, med_true))
    assert share < 0.05
    assert med_nz > 10 * med_true      # one float ulp (>= 1.5e-5 at >= 128 pixels) / 2e-9


# ---- recovery and policy
def recovery_runs():
    """150 noise-free pairs, no outliers, the start 2 degrees / 5 % of the translation / 5 % of the scale off the truth, th2 = 10 as LoopClosing calls
    it -> (start distances, {mode: (result, end distances)})"""
    c = sc.case(31, N=150, outliers=0.0, noise_px=0.0, fix_scale=0, start_deg=2.0, start_t=0.05, start_s=0.05)
    d0 = sc.distances(c, ref.quat_from_R(c["R12"]), c["t12"], c["s12"])
    out = {}
    for mode in (1, 0):
        rc, got = hl.optimize_host(F, [api.sim3_opt_job_state(c, sc.TH2, jacobian=mode)])
        assert rc == 0
        r = got[0]
        out[mode] = (r, sc.distances(c, r["q12"], r["t12"], r["s12"][0]))
    return d0, out


def test_recovery_with_the_analytic_jacobian():
    """The analytic mode brings the estimate closer to the truth in rotation, translation and scale and keeps every pair; the as-written mode on the
    same start is printed, not asserted"""
    d0, out = recovery_runs()
    for mode in (1, 0):
        r = out[mode][0]
        print("recovery, jacobian %d: start (rot %.3g rad, |dt| %.3g, ds %.3g) -> end (%.3g, %.3g, %.3g), %d of 150 kept, iterations %s"
              % ((mode,) + d0 + out[mode][1] + (r["n_inliers"], list(r["iterations"]))))
    r, d1 = out[1]
    assert r["n_inliers"] == 150 and r["keep"].all() and r["n_bad"] == 0
    assert d1[0] < d0[0] and d1[1] < d0[1] and d1[2] < d0[2]
    # (the as-written run above is recorded, not asserted)


def test_policy_paths():
    # fewer than 10 survivors: 0 and the estimate untouched
    for N, outl in ((9, 0.0), (14, 0.9)):
        c = sc.case(40 + N, N=N, outliers=outl)
        for mode in (0, 1):
            r = hl.optimize_host(F, [api.sim3_opt_job_state(c, sc.TH2, jacobian=mode)])[1][0]
            assert r["n_correspondences"] - r["n_bad"] < 10 and r["n_inliers"] == 0 and r["iterations"][1] == 0
            assert bits(r["q12"]) == bits(ref.quat_from_R(c["R12"])) and bits(r["t12"]) == bits(c["t12"]) and r["s12"][0] == c["s12"]
            assert int(r["keep"].sum()) == N - r["n_bad"]
    # nBad == 0 takes 5 further iterations at the most, nBad > 0 up to 10 -- and more than 5 somewhere, or the 10 would not show
    seen_more = False
    for seed in range(50, 58):
        for outl in (0.0, 0.3):
            c = sc.case(seed, N=120, outliers=outl, noise_px=0.5 if outl else 0.05)
            for mode in (0, 1):
                r = hl.optimize_host(F, [api.sim3_opt_job_state(c, sc.TH2, jacobian=mode)])[1][0]
                assert 1 <= r["iterations"][0] <= 5
                if r["n_bad"] == 0:
                    assert r["iterations"][1] <= 5
                else:
                    assert r["iterations"][1] <= 10
                    seen_more |= r["iterations"][1] > 5
                assert r["n_inliers"] == int(r["keep"].sum()) <= 120 - r["n_bad"]
    assert seen_more


def test_checks_refuse_with_a_reason():
    c = sc.case(60, N=20)
    def rc_of(**kw):
        s = api.sim3_opt_job_state(c, sc.TH2); s.update(kw)
        arr = api.sim3_opt_jobs([s])
        rc = hl.H().hm_sim3_optimize_host(F, 1, arr)
        assert arr[0].n_inliers == -7 and (s["keep"] == 7).all()
        return rc, hl.H().hm_sim3_opt_last_reason().decode()
    for kw in (dict(th2=0.0), dict(th2=float("nan")), dict(s12=-1.0), dict(s12=float("inf")), dict(jacobian=2), dict(kp1=None)):
        rc, why = rc_of(**kw)
        assert rc != 0 and why, kw
    s = api.sim3_opt_job_state(c, sc.TH2); s["kp2"][5] = (5.0, 5.0)      # a corner block of the cubemap image
    assert hl.H().hm_sim3_optimize_host(F, 1, api.sim3_opt_jobs([s])) != 0 and b"no face" in hl.H().hm_sim3_opt_last_reason()


# ---- ABI
def test_abi_matches_the_header(tmp_path):
    L = api.lib()
    for name in ("cms_sim3_opt_create", "cms_sim3_opt_destroy", "cms_sim3_optimize"):
        assert hasattr(L, name), name
    assert hasattr(hl.H(), "hm_sim3_optimize_host")
    fields = [f[0] for f in api.Sim3OptJob._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cubemapslam_hip.h"\nint main(void) {\n  printf("%zu", sizeof(cms_sim3_opt_job));\n' +
                   "".join('  printf(" %%zu", offsetof(cms_sim3_opt_job, %s));\n' % f for f in fields) +
                   '  printf(" %d %d", CMS_SIM3_OPT_AS_WRITTEN, CMS_SIM3_OPT_ANALYTIC);\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(api.Sim3OptJob) and out[1:-2] == [getattr(api.Sim3OptJob, f).offset for f in fields]
    assert out[-2:] == [api.SIM3_OPT_AS_WRITTEN, api.SIM3_OPT_ANALYTIC]


# ---- the mirror class over HOST_CORE
@pytest.mark.parametrize("jacobian", (0, 1))
def test_mirror_over_host_core(jacobian):
    """Optimizer::OptimizeSim3 of cubemap_hot_path.h on a case with holes, bad points and points without an index: the graph
    it collects is the literal rule's (:941-978), the rest is hm_sim3_optimize_host on those arrays, and vpMatches1 loses exactly the pairs the call drops"""
    import sim3_hostlib
    camd, kf1, kf2, m12, start = hl.mirror_case()
    want = hl.mirror_expected_graph(kf1, kf2, m12)
    _, _, _, _, kept_by_solver = sim3_hostlib.mirror_case()
    # the case exercises every skip, and OptimizeSim3's filter is not Sim3Solver's: no index test on key frame 1's side, no projection test
    m = np.asarray(m12); mp1 = kf1["mp"]
    assert (m < 0).any() and ((m >= 0) & (mp1 < 0)).any() and kf1["bad"].any() and kf2["bad"].any() and (kf2["index_in_kf"][m[m >= 0]] < 0).any()
    assert set(kept_by_solver.tolist()) < set(want["idx"].tolist()) and len(want["idx"]) >= len(kept_by_solver) + 6
    got = hl.mirror(1, camd, kf1, kf2, m12, start, sc.TH2, False, jacobian)
    assert got["N"] == len(want["idx"]) and np.array_equal(got["idx"], want["idx"])
    for k in ("x3dc1", "x3dc2", "kp1", "kp2", "inv_sigma2_1", "inv_sigma2_2"):
        assert np.asarray(got[k], np.float32).tobytes() == np.ascontiguousarray(want[k], np.float32).tobytes(), k
    job = dict(want, R12=start["R12"], t12=start["t12"], s12=start["s12"])
    rc, ref_run = hl.optimize_host(F, [api.sim3_opt_job_state(job, sc.TH2, fix_scale=0, jacobian=jacobian)])
    assert rc == 0
    r = ref_run[0]
    assert got["n_inliers"] == r["n_inliers"] and bits(got["q12"]) == bits(r["q12"]) and bits(got["t12"]) == bits(r["t12"]) and bits(got["s12"]) == bits(r["s12"])
    expect = m.copy()
    expect[want["idx"][r["keep"] == 0]] = -1
    assert np.array_equal(got["matches1"], expect)
    assert 0 < int((r["keep"] == 0).sum()) < len(want["idx"]) and r["n_inliers"] >= 20      # some pairs go (the outliers), most stay
