"""Sim3Solver without a GPU: the shared core (cubemapslam_amd/csrc/cms_sim3_core.h) as the host build runs it (libcubemapslam_host.so), pinned from
outside stage by stage against an independent float64 restatement with np.linalg.eigh (tests/npref_sim3.py), by properties of the motion, and by a
bit-exact restatement of CheckInliers; the loop of Sim3Solver::iterate on hand-made problems; cms_sim3_ransac_parameters; the job check; the ABI; the
core header built on its own, also as a stand-alone program under the host sanitizers.

Bars.  A stage the core computes in double is held to 1e-9 (relative to the stage's magnitude), as in the PnP tests.  A stage the reference stores as
CV_32F is the double value rounded to float: U = 2^-24 relative per rounding, counted per stage below.  R depends on the eigenvector, whose
conditioning is the relative eigengap (lambda1 - lambda2) / |lambda1|: the bar is |dR| * gap <= 4 * B over the hypotheses with gap >= 1e-2, where B
is the same quantity between a float32 and a float64 run of the restatement itself on the same hypotheses (measured in the fixture, independent of
the core; 2.4e-7 on these cases) and 4 is the margin for another eigen-solver and summation order (profiles/sim3.md)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import npref_sim3 as ref
import sim3_cases as sc
import sim3_hostlib as hl
from cubemapslam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = sc.F
U = 2.0 ** -24
PROBLEMS = ((55, 0.3, 20), (90, 0.4, 25), (130, 0.5, 30), (180, 0.35, 35), (240, 0.5, 40), (64, 0.45, 20))      # N, outliers, min_inliers
KEYS_I = ("status", "no_more", "n_inliers", "iterations", "iterations_run", "best_inliers")


@pytest.fixture(scope="module")
def hypotheses():
    """6 problems x 300 hypotheses: (problem, triple, the core's stages, the restatement in float64 and in float32 from the raw points)"""
    out = []
    for j, (N, o, mi) in enumerate(PROBLEMS):
        pr = sc.problem(300 + j, N=N, outliers=o, min_inliers=mi)
        for row in sc.draws(400 + j, N, 300):
            idx = sc.swap_and_pop(N, row)
            P1, P2 = pr["x3dc1"][idx], pr["x3dc2"][idx]
            out.append((pr, idx, hl.compute(P1, P2), ref.compute_sim3(P1, P2, dt=np.float64), ref.compute_sim3(P1, P2, dt=np.float32)))
    return out


def test_stage_by_stage_against_the_restatement(hypotheses):
    B = 0.0
    for _, _, g, a, b in hypotheses:
        if a["gap"] >= 1e-2:
            B = max(B, np.abs(a["R"] - b["R"].astype(np.float64)).max() * a["gap"])
    print("B (float32 against float64 restatement, |dR| * gap) = %.3e" % B)
    assert 1e-8 < B < 1e-6                      # the measurement itself is sane: a few float roundings
    left_out, worst_R = 0, 0.0
    for pr, idx, g, _, _ in hypotheses:
        P1, P2 = pr["x3dc1"][idx].astype(np.float64), pr["x3dc2"][idx].astype(np.float64)
        # centroid and relative coordinates (float): two additions and a division, then one subtraction -> 4 U of the coordinates' magnitude
        for P, Pr, O in ((P1, g["Pr1"], g["O1"]), (P2, g["Pr2"], g["O2"])):
            rPr, rO = ref.centroid(P.T)
            mag = np.abs(P).max()
            assert np.abs(O - rO).max() <= 3 * U * mag and np.abs(Pr - rPr).max() <= 4 * U * mag
        # M from the core's Pr: a double sum rounded once
        rM = ref.m_matrix(g["Pr1"], g["Pr2"])
        assert (np.abs(g["M"] - rM) <= U * np.abs(rM) + 1e-9 * np.abs(rM).max()).all()
        # N from the core's M: double sums of floats, stored as float -> the rounded restatement exactly
        rN = ref.n_matrix(g["M"])
        assert np.array_equal(g["N"], rN.astype(np.float32))
        # eigenvalues (double Jacobi) from the core's N
        e, w = ref.top_eigenvector(g["N"])
        scale = np.abs(w).max()
        if scale > 0:
            assert np.abs(np.sort(g["evals"])[::-1] - w).max() <= 1e-9 * scale
        assert g["evals"][g["chosen"]] == g["evals"].max() and g["chosen"] == int(np.argmax(g["evals"]))      # first maximum wins
        assert np.array_equal(g["q"], g["evecs"][:, g["chosen"]].astype(np.float32))
        gap = ref.relative_gap(w)
        # R from the core's N through eigh, atan2 and Rodrigues
        if gap >= 1e-2:
            v = np.abs(g["R"] - ref.rotation(e)).max() * gap
            worst_R = max(worst_R, v)
            assert v <= 4 * B, (v, B, gap)
        else:
            left_out += 1
        # scale from the core's Pr1, Pr2 and R: P3 is rounded to float (U per entry), its squares once more
        s, P3, nom, den = ref.scale(g["Pr1"], g["Pr2"], g["R"])
        terms = (np.abs(g["Pr1"].astype(np.float64)) * np.abs(P3)).sum()
        assert abs(g["nom"] - nom) <= 2 * U * terms + 1e-9 * terms
        assert abs(g["den"] - den) <= 4 * U * den + 1e-9 * den
        with np.errstate(all="ignore"):
            want_s = np.float32(g["nom"] / g["den"])
        assert g["s"].view(np.uint32) == (want_s.view(np.uint32) if want_s == want_s else 0x7FC00000)      # a NaN leaves the core as the one quiet NaN
        if not np.isfinite(g["s"]):
            continue
        # t from the core's O1, O2, R, s: the product rounded to float, then a float subtraction
        rt = ref.translation(g["O1"], g["O2"], g["R"], g["s"])
        mag = np.abs(g["O1"]).max() + abs(float(g["s"])) * np.abs(g["R"].astype(np.float64)).sum(1).max() * np.abs(g["O2"]).max()
        assert np.abs(g["t"] - rt).max() <= 2 * U * mag
        # T12, T21 from the core's R, t, s: one rounding per entry of sR and of (1/s) R^T; tinv sums three products of rounded entries
        T12, T21 = ref.transforms(g["R"], g["t"], g["s"])
        assert (np.abs(g["T12"] - T12) <= U * np.abs(T12) + 1e-12).all()
        assert (np.abs(g["T21"][:, :3] - T21[:, :3]) <= U * np.abs(T21[:, :3]) + 1e-12).all()
        mag = (np.abs(T21[:, :3]) * np.abs(g["t"].astype(np.float64))[None, :]).sum(1)
        assert (np.abs(g["T21"][:, 3] - T21[:, 3]) <= 3 * U * mag + 1e-12).all()
    print("|dR| * gap core against restatement: %.3e (bar %.3e); %d of %d hypotheses below the gap bound" % (worst_R, 4 * B, left_out, len(hypotheses)))
    assert len(hypotheses) == 1800 and left_out <= 0.05 * len(hypotheses)


def test_inlier_masks_equal_the_numpy_restatement_everywhere(hypotheses):
    """CheckInliers of the core on the core's own T12 / T21 against the float32-step restatement: equal for every correspondence, no exclusions"""
    total = inl = 0
    for pr, idx, g, _, _ in hypotheses:
        a = hl.check_inliers(F, g["T12"], g["T21"], pr["x3dc1"], pr["x3dc2"], pr["max_err1"], pr["max_err2"])
        b = ref.check_inliers(F, g["T12"], g["T21"], pr["x3dc1"], pr["x3dc2"], pr["max_err1"], pr["max_err2"])
        assert np.array_equal(a, b)
        total += len(a); inl += int(a.sum())
    assert total > 150000 and 5000 < inl < total // 2, (total, inl)


def test_motion_properties(hypotheses):
    """R orthonormal with det +1 within the bar of the rotation stage; T21 T12 = I to float rounding: each entry of either matrix carries one
    rounding, a row-by-column product sums four terms -> 8 U of the terms' magnitude"""
    B4 = 4 * 2.5e-7
    for _, _, g, _, _ in hypotheses[::3]:
        if not np.isfinite(g["s"]) or g["s"] == 0:
            continue
        R = g["R"].astype(np.float64)
        assert np.abs(R.T @ R - np.eye(3)).max() <= B4 and abs(np.linalg.det(R) - 1) <= B4
        A = np.vstack([g["T21"].astype(np.float64), [0, 0, 0, 1]]); Bm = np.vstack([g["T12"].astype(np.float64), [0, 0, 0, 1]])
        mag = np.abs(A) @ np.abs(Bm)
        assert (np.abs(A @ Bm - np.eye(4)) <= 8 * U * mag).all()


def test_noise_free_triples_recover_the_truth():
    """Exact correspondences stored as float32 (dX <= 2^-24 * 8 m = 4.8e-7 per coordinate).  A triangle whose smallest altitude is h turns by at most
    about 2 sqrt(3) dX / h: with h >= 0.5 m that is 3.3e-6; the bar is 1e-5 for R and s and 1e-5 * (1 + |O2|) <= 1e-4 for t"""
    used = 0
    for seed in range(20, 26):
        pr = sc.problem(seed, N=40, outliers=0.0, noise=0.0)
        for row in sc.draws(seed + 50, 40, 30):
            idx = sc.swap_and_pop(40, row)
            P = pr["x3dc1"][idx].astype(np.float64)
            sides = [np.linalg.norm(P[a] - P[b]) for a, b in ((0, 1), (1, 2), (2, 0))]
            area2 = np.linalg.norm(np.cross(P[1] - P[0], P[2] - P[0]))
            if area2 / max(sides) < 0.5:
                continue
            used += 1
            g = hl.compute(pr["x3dc1"][idx], pr["x3dc2"][idx])
            assert np.abs(g["R"] - pr["R12"]).max() <= 1e-5 and abs(g["s"] - pr["s12"]) <= 1e-5 and np.abs(g["t"] - pr["t12"]).max() <= 1e-4
            m = hl.check_inliers(F, g["T12"], g["T21"], pr["x3dc1"], pr["x3dc2"], pr["max_err1"], pr["max_err2"])
            assert m.all()
    assert used > 60


def test_fix_scale_is_exactly_one():
    pr = sc.problem(7, N=30, outliers=0.0)
    g = hl.compute(pr["x3dc1"][:3], pr["x3dc2"][:3], fix_scale=True)
    assert g["s"].view(np.uint32) == np.float32(1.0).view(np.uint32) and g["nom"] == 0 and g["den"] == 0
    assert np.array_equal(g["T12"][:, :3], g["R"]) and np.array_equal(g["T21"][:, :3], g["R"].T)
    free = hl.compute(pr["x3dc1"][:3], pr["x3dc2"][:3])
    assert free["s"] != 1 and np.array_equal(free["R"], g["R"])


def test_degenerate_triples_finish_and_nan_is_no_inlier():
    pr = sc.problem(8, N=30, outliers=0.0)
    x1, x2 = pr["x3dc1"], pr["x3dc2"]
    # coincident: M = 0, R = I, den = 0 -> s = NaN
    g = hl.compute(np.repeat(x1[:1], 3, 0), np.repeat(x2[:1], 3, 0))
    assert np.isnan(g["s"]) and np.array_equal(g["R"], np.eye(3, dtype=np.float32)) and g["sweeps"] == 0
    assert g["s"].view(np.uint32) == 0x7FC00000 and (g["T12"][:, :3].view(np.uint32) == 0x7FC00000).all()      # the NaN bits are the same on every build
    assert not hl.check_inliers(F, g["T12"], g["T21"], x1, x2, pr["max_err1"], pr["max_err2"]).any()
    assert not ref.check_inliers(F, g["T12"], g["T21"], x1, x2, pr["max_err1"], pr["max_err2"]).any()
    # collinear: the rotation about the line is free, something finite and orthonormal comes out
    line1 = (x1[0][None, :] + np.array([[0.0], [0.5], [1.25]]) * (x1[1] - x1[0])[None, :]).astype(np.float32)
    line2 = (x2[0][None, :] + np.array([[0.0], [0.5], [1.25]]) * (x2[1] - x2[0])[None, :]).astype(np.float32)
    g = hl.compute(line1, line2)
    R = g["R"].astype(np.float64)
    assert np.isfinite(g["T12"]).all() and np.abs(R.T @ R - np.eye(3)).max() < 1e-6 and g["sweeps"] < 16
    # NaN and inf coordinates: the Jacobi stops, everything is NaN, nobody is an inlier
    bad = x1[:3].copy(); bad[1, 2] = np.nan
    g = hl.compute(bad, x2[:3])
    assert np.isnan(g["T12"]).any() and g["sweeps"] == 0
    assert not hl.check_inliers(F, g["T12"], g["T21"], x1, x2, pr["max_err1"], pr["max_err2"]).any()
    bad = x1[:3].copy(); bad[0, 0] = np.inf
    g = hl.compute(bad, x2[:3])
    assert not hl.check_inliers(F, g["T12"], g["T21"], x1, x2, pr["max_err1"], pr["max_err2"]).any()
    # as a job: every hypothesis of a job of identical points is NaN, the loop walks them all
    same_pts = dict(pr, x3dc1=np.repeat(x1[:1], 30, 0), x3dc2=np.repeat(x2[:1], 30, 0), min_inliers=5, max_its=12)
    rc, res = hl.iterate_host(F, [api.sim3_job_state(same_pts, 12, sc.draws(9, 30, 12))])
    assert rc == 0 and res[0]["status"] == 0 and res[0]["no_more"] == 1 and res[0]["iterations"] == 12 and res[0]["best_inliers"] == 0
    assert np.isnan(res[0]["best_s"][0])      # 0 >= 0: the last NaN hypothesis is the best


def test_jacobi_on_symmetric_matrices():
    rng = np.random.default_rng(3)
    for k in range(40):
        A = rng.normal(size=(4, 4)); A = A + A.T
        if k % 4 == 0:
            A[2] = A[1]; A[:, 2] = A[:, 1]      # a repeated eigenvalue
        w, V, n = hl.jacobi4(A)
        assert n < 16 and np.abs(V.T @ V - np.eye(4)).max() < 1e-14 and np.abs(A @ V - V * w[None, :]).max() < 1e-13 * np.abs(A).max() * 10
        assert np.abs(np.sort(w) - np.linalg.eigvalsh(A)).max() < 1e-13 * np.abs(A).max() * 10
    w, V, n = hl.jacobi4(np.diag([1.0, 5.0, 5.0, 2.0]))
    assert n == 0 and np.array_equal(V, np.eye(4))


def test_quaternion_rotation_equals_atan2_rodrigues():
    """The rotation built from the quaternion's products is the one atan2 -> angle-axis -> Rodrigues gives, for either sign and any length of the
    vector, also beyond a half turn (negative real part)"""
    rng = np.random.default_rng(4)
    for k in range(200):
        q = rng.normal(size=4).astype(np.float32) * np.float32(rng.uniform(0.1, 3))
        if k % 5 == 0:
            q[0] = -abs(q[0])
        R = hl.quat_to_R(q)
        assert np.abs(R - ref.rotation(q.astype(np.float64))).max() <= 4 * U
        assert np.array_equal(R, hl.quat_to_R(-q))


def test_draws_resolve_like_swap_and_pop():
    rng = np.random.default_rng(5)
    for N in (3, 4, 5, 9, 64):
        for _ in range(60):
            row = [int(rng.integers(0, N - k)) for k in range(3)]
            assert hl.resolve_draws(N, row) == sc.swap_and_pop(N, row)
        for row in ((N - 1, N - 2, N - 3), (0, 0, 0), (N - 1, 0, N - 3), (0, N - 2, 0)):
            assert hl.resolve_draws(N, row) == sc.swap_and_pop(N, row)


# ---------------------------------------------------------------------------------------------------------------- the loop

N_IN, N_OUT = 12, 8


def hand_built():
    """12 exact correspondences, 8 far outliers, and two different inlier triples whose hypotheses have the same 12 inliers and different T12"""
    pr = sc.exact_problem(5, N_IN, N_OUT)
    N = N_IN + N_OUT
    triples = [t for t in ((0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (0, 4, 8), (1, 5, 9))]
    good = []
    for t in triples:
        g = hl.compute(pr["x3dc1"][list(t)], pr["x3dc2"][list(t)])
        m = hl.check_inliers(F, g["T12"], g["T21"], pr["x3dc1"], pr["x3dc2"], pr["max_err1"], pr["max_err2"])
        if m.sum() == N_IN and m[:N_IN].all():
            good.append((t, g))
    assert len(good) >= 2 and not np.array_equal(good[0][1]["T12"], good[1][1]["T12"])
    outlier_triple = (0, N_IN, N_IN + 1)
    return pr, N, good[0], good[1], outlier_triple


def run_host(pr, n_iterations, d, **kw):
    st = api.sim3_job_state(dict(pr, **kw), n_iterations, d)
    rc, res = hl.iterate_host(F, [st])
    return rc, (res[0] if rc == 0 else None), st


def test_tie_replaces_the_best():
    """mnInliersi >= mnBestInliers (:207): of two hypotheses with the same count the SECOND is the best (PnPsolver keeps the first)"""
    pr, N, (t1, g1), (t2, g2), _ = hand_built()
    d = sc.draws_for([t1, t2], N)
    rc, r, _ = run_host(pr, 2, d, min_inliers=15, max_its=2)
    assert rc == 0 and r["status"] == 0 and r["no_more"] == 1 and r["best_inliers"] == N_IN and r["iterations"] == 2
    assert np.array_equal(r["best_T12"], g2["T12"].ravel()) and not np.array_equal(r["best_T12"], g1["T12"].ravel())
    assert np.array_equal(r["best_R"], g2["R"].ravel()) and np.array_equal(r["best_t"], g2["t"]) and r["best_s"][0] == g2["s"]
    assert not r["inliers"].any() and not r["T12"].any()


def test_exactly_min_inliers_is_the_best_but_not_accepted():
    pr, N, (t1, g1), _, bad = hand_built()
    d = sc.draws_for([bad, t1, bad], N)
    rc, r, _ = run_host(pr, 3, d, min_inliers=N_IN, max_its=3)
    assert rc == 0 and r["status"] == 0 and r["best_inliers"] == N_IN and r["iterations"] == 3 and r["no_more"] == 1
    assert np.array_equal(r["best_T12"], g1["T12"].ravel()) and r["best_mask"][:N_IN].all() and not r["best_mask"][N_IN:].any()
    rc, r, _ = run_host(pr, 3, d, min_inliers=N_IN - 1, max_its=3)      # one below: accepted at once, the third draw is never used
    assert r["status"] == 1 and r["n_inliers"] == N_IN and r["iterations"] == 2 and r["iterations_run"] == 2 and r["no_more"] == 0
    assert np.array_equal(r["T12"], g1["T12"].ravel()) and np.array_equal(r["inliers"], r["best_mask"]) and r["inliers"].sum() == N_IN


def test_fewer_correspondences_than_min_inliers():
    pr = sc.problem(11, N=7, outliers=0.0)
    st = api.sim3_job_state(dict(pr, min_inliers=20, max_its=300, iterations=3, best_T12=np.arange(12)), 5, [])
    rc, res = hl.iterate_host(F, [st])
    r = res[0]
    assert rc == 0 and r["no_more"] == 1 and r["status"] == 0 and r["iterations"] == 3 and r["iterations_run"] == 0 and np.array_equal(r["best_T12"], np.arange(12, dtype=np.float32))


def test_carried_best_with_a_higher_count_stays():
    pr, N, (t1, g1), (t2, _), _ = hand_built()
    mask = np.zeros(N, np.uint8); mask[:6] = 1; mask[N_IN:N_IN + 7] = 1
    carried = dict(best_inliers=13, best_mask=mask, best_T12=np.arange(12), best_R=np.arange(9), best_t=np.arange(3), best_s=2.5, iterations=4)
    rc, r, _ = run_host(pr, 2, sc.draws_for([t1, t2], N), min_inliers=10, max_its=6, **carried)
    assert rc == 0 and r["status"] == 0 and r["best_inliers"] == 13 and np.array_equal(r["best_mask"], mask) and r["iterations"] == 6 and r["no_more"] == 1
    assert np.array_equal(r["best_T12"], np.arange(12, dtype=np.float32)) and r["best_s"][0] == 2.5 and np.array_equal(r["best_R"], np.arange(9, dtype=np.float32))
    # 12 carried: the hypothesis with 12 replaces it and, above min_inliers, is accepted
    mask12 = mask.copy(); mask12[0] = 0
    rc, r, _ = run_host(pr, 2, sc.draws_for([t1, t2], N), min_inliers=10, max_its=6, **dict(carried, best_inliers=12, best_mask=mask12))
    assert r["status"] == 1 and r["iterations"] == 5 and np.array_equal(r["T12"], g1["T12"].ravel())


def test_the_while_condition_and_two_calls_equal_one():
    """while (mnIterations < max_its && nCurrentIterations < n_iterations): a call runs min(max_its - iterations, n_iterations); 10 + the rest = one call"""
    pr = sc.problem(12, N=25, outliers=0.3, min_inliers=20, max_its=40)      # 25 correspondences at 30 % outliers never pass 20
    d = sc.draws(13, 25, 40)
    rc, one, _ = run_host(pr, 40, d)
    assert rc == 0 and one["status"] == 0 and one["no_more"] == 1 and one["iterations"] == 40 and 3 <= one["best_inliers"] <= 20
    rc, a, _ = run_host(pr, 10, d)
    assert a["iterations"] == 10 and a["iterations_run"] == 10 and a["no_more"] == 0
    carry = {k: a[k] for k in ("iterations", "best_inliers", "best_mask", "best_T12", "best_R", "best_t")}
    rc, b, _ = run_host(pr, 30, d[10:], best_s=a["best_s"][0], **carry)
    assert b["iterations_run"] == 30
    assert api.sim3_first_difference([one], [dict(b, iterations_run=one["iterations_run"])]) is None
    rc, c, _ = run_host(pr, 0, d)
    assert rc == 0 and c["iterations"] == 0 and c["no_more"] == 0 and c["status"] == 0


def test_ransac_parameters():
    assert api.sim3_ransac_parameters(100, 0.99, 20, 300) == 300
    for N, mi, mx in ((100, 20, 300), (40, 20, 300), (25, 20, 300), (21, 20, 300), (20, 20, 300), (19, 20, 300), (0, 20, 300), (0, 0, 300), (7, 6, 5), (300, 6, 300),
                      (50, 45, 300), (3, 3, 10), (60, 20, 0)):
        assert api.sim3_ransac_parameters(N, 0.99, mi, mx) == ref.ransac_parameters(N, 0.99, mi, mx), (N, mi, mx)
    assert api.sim3_ransac_parameters(20, 0.99, 20, 300) == 1          # minInliers == N
    assert api.sim3_ransac_parameters(19, 0.99, 20, 300) == 1          # epsilon > 1: the log of a negative number, NaN -> INT_MIN -> 1
    assert api.sim3_ransac_parameters(0, 0.99, 20, 300) == 1           # N = 0: epsilon = inf
    assert api.sim3_ransac_parameters(40, 0.99, 20, 300) == 35
    assert api.sim3_ransac_parameters(40, 0.5, 20, 300) == 6


def test_job_check_refuses_and_leaves_the_records():
    pr = sc.problem(1, N=30, outliers=0.2, min_inliers=10, max_its=5)
    d = sc.draws(2, 30, 5)

    def refused(n_iterations, draws, **kw):
        st = api.sim3_job_state(dict(pr, **kw), n_iterations, draws)
        st["inliers"][:] = 7
        arr = api.sim3_jobs([st])
        arr[0].status = 99; arr[0].n_inliers = 98
        before = bytes(arr[0])
        rc = hl.H().hm_sim3_iterate_host(F, 1, arr)
        untouched = bytes(arr[0]) == before and (st["inliers"] == 7).all()
        return rc, untouched
    e = d.copy(); e[3, 0] = 30
    assert refused(5, e) == (-1, True)                                  # draw 0 outside [0, N-1]
    e = d.copy(); e[4, 2] = 28
    assert refused(5, e) == (-1, True)                                  # draw 2 outside [0, N-3]
    e = d.copy(); e[1, 1] = -1
    assert refused(5, e) == (-1, True)
    assert refused(5, d[:4]) == (-1, True)                              # n_draws < 3 * max(max_its - iterations, n_iterations)
    assert refused(7, sc.draws(2, 30, 6)) == (-1, True)                 # ... with n_iterations the larger of the two
    assert refused(5, d, best_inliers=2) == (-1, True)                  # best_mask against best_inliers
    assert refused(5, d, min_inliers=2) == (-1, True)                   # min_inliers < 3
    assert refused(5, d, max_its=-1) == (-1, True)
    assert refused(5, sc.draws(2, 30, 5), max_its=(1 << 20) + 1) == (-1, True)
    assert refused(-1, d) == (-1, True)
    assert refused((1 << 20) + 1, d) == (-1, True)
    rc, ok = refused(5, d)
    assert rc == 0 and not ok
    rc, ok = refused(5, d[:3], iterations=2)                            # two iterations behind: three left, but n_iterations = 5 asks for 15 draws
    assert rc == -1
    assert refused(3, d[:3], iterations=2)[0] == 0
    assert refused(5, [], min_inliers=31)[0] == 0                       # N < min_inliers: no draw is needed


def test_exports_and_job_layout(tmp_path):
    L = api.lib()
    for name in ("cms_sim3_ransac_parameters", "cms_sim3_create", "cms_sim3_destroy", "cms_sim3_iterate"):
        assert hasattr(L, name), name
    assert hasattr(hl.H(), "hm_sim3_iterate_host")
    fields = [f[0] for f in api.Sim3Job._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cubemapslam_hip.h"\nint main(void) {\n  printf("%zu", sizeof(cms_sim3_job));\n' +
                   "".join('  printf(" %%zu", offsetof(cms_sim3_job, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(api.Sim3Job) and out[1:] == [getattr(api.Sim3Job, f).offset for f in fields]


EMU = os.path.join(ROOT, "tests", "emu", "sim3_core_emu.cpp")
GPP = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "cubemapslam_amd", "csrc")]


def test_core_header_alone_under_gpp(tmp_path, hypotheses):
    """cms_sim3_core.h compiled on its own by g++ (tests/emu/sim3_core_emu.cpp) gives the host library's bits, stage for stage"""
    so = tmp_path / "sim3_core_emu.so"
    subprocess.check_call(GPP + ["-O2", "-fPIC", "-shared", EMU, "-o", str(so)])
    E = C.CDLL(str(so))
    E.emu_sim3_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    E.emu_sim3_compute.restype = None
    assert E.emu_stages_size() == C.sizeof(hl.Stages) and E.emu_motion_size() == C.sizeof(hl.Motion)
    for pr, idx, g, _, _ in hypotheses[::37]:
        e = hl.compute(pr["x3dc1"][idx], pr["x3dc2"][idx], lib=E, name="emu_sim3_compute")
        for k in g:
            assert np.asarray(g[k]).tobytes() == np.asarray(e[k]).tobytes(), k


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """-DSIM3_EMU_MAIN: a program with its own main, built with -fsanitize=address,undefined and run on a case file with ordinary, coincident,
    collinear, NaN and inf triples.  Nothing of it is loaded into this process."""
    exe = tmp_path / "sim3_core_emu"
    subprocess.check_call(GPP + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                                 "-DSIM3_EMU_MAIN", EMU, "-o", str(exe)])
    cases = []
    for seed in range(12):
        pr = sc.problem(60 + seed, N=20 + seed, outliers=0.3, fix_scale=seed % 2 if seed >= 8 else 0)
        x1, x2 = pr["x3dc1"].copy(), pr["x3dc2"].copy()
        if seed == 3:
            x1[:3] = x1[0]; x2[:3] = x2[0]
        elif seed == 4:
            x1[2] = x1[0] + 2 * (x1[1] - x1[0]); x2[2] = x2[0] + 2 * (x2[1] - x2[0])
        elif seed == 5:
            x1[1, 1] = np.nan
        elif seed == 6:
            x2[0, 2] = np.inf
        elif seed == 7:
            x1[:] = 0; x2[:] = 0
        cases.append((len(x1), pr["fix_scale"], x1, x2, pr["max_err1"], pr["max_err2"]))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for n, fix, x1, x2, m1, m2 in cases:
            f.write(struct.pack("<iii", n, F, fix))
            for a in (x1, x2, m1, m2):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.startswith("12 cases, ") and " NaN motions" in r.stdout
    assert int(r.stdout.split(",")[1].split()[0]) >= 3      # NaN, inf and all-zero inputs; coincident points may leave a rounding residue of the centroid instead
