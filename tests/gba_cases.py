"""Cases and measures shared by tests/test_global_ba_cpu.py and tests/test_gpu_global_ba.py.

The bar is the project's: every block's update -- a key frame's translation, a key frame's rotation, a point, each on its
own -- within 1e-4 of the reference's update of that block, with a floor of 1 % of the median update.  Windows whose POINTS cascade at
float-rounding level in the reference itself (the residual goes through a float) are held to the cascade-aware bar: key frames strictly, points
no worse than the reference against itself under a 1e-12 m perturbation (three times as many beyond the bar, five times the worst value).
Restated from tests/test_gpu_parity.py::_ba_updates_close / _ba_updates_close_or_cascade so that no test file imports another."""
import functools

import numpy as np

from cubemapslam_amd import synth
import npref_global_ba as npref
import orc

TOL = 1e-4

# name -> synth.ba_problem arguments.  strict: the reference agrees with itself within the bar under a 1e-12 m perturbation;
# cascade: its points do not (key frames do), counted by the tests.
CASES = {
    "K2": dict(K=2, P=300, obs_per_point=2, F=650, seed=13),
    "K3": dict(K=3, P=400, obs_per_point=3, F=650, seed=12),
    "K33": dict(K=33, P=1500, obs_per_point=5, F=550, seed=31),
    "K34": dict(K=34, P=1500, obs_per_point=5, F=550, seed=22),
    "K40": dict(K=40, P=2500, obs_per_point=6, F=550, seed=4),
    "K40r": dict(K=40, P=2500, obs_per_point=6, F=550, seed=6),
    "K65": dict(K=65, P=3000, obs_per_point=6, F=550, seed=32),
    "K130": dict(K=130, P=5000, obs_per_point=6, F=550, seed=34),
}
# Seeds swapped after measuring (test_global_ba_cpu.py re-measures all of them): with the kernel width of BundleAdjustment's text, sqrt(5.99), the
# K = 34 seed 21 and K = 40 seed 4 windows cascade on points against themselves (11 and 21 points beyond 1e-4, worst 2.2e-4 and 4.7e-4; key frames
# <= 5e-6), so the strict robust cases are seed 22 (worst block 2e-9) and seed 6 (3e-9).  K = 40 seed 4 stays the window without kernel (2e-9) and the
# two-stage guard.  K = 65 seed 32 turned out tame at this width (2e-9), K = 130 seed 34 cascades (48 points, worst 8e-4, key frames 8e-6): both
# are held to the cascade-aware bar and counted.
STRICT = ("K2", "K3", "K33", "K34", "K40r")
CASCADE = ("K65", "K130")
ROBUST_ITS = 20
PLAIN_ITS = 10
PLAIN_CANDIDATES = ("K3", "K33", "K40")      # robust = 0: the CPU test decides which of them the GPU test may use ...
PLAIN_ADMITTED = ("K3", "K40")               # ... these (K33 seed 31 without kernel: 6 points beyond 1e-4 against itself, worst 1.8e-4)


@functools.lru_cache(maxsize=None)
def problem(name):
    return synth.ba_problem(**CASES[name])


def perturbed(prob):
    rs = np.random.RandomState(1)
    p2 = dict(prob)
    p2["points"] = prob["points"] + rs.normal(0, 1e-12, prob["points"].shape)
    return p2


def block_errors(prob, got_poses, got_points, want_poses, want_points):
    """per block |got - want| relative to max(|want's update|, 1 % of the median update): (translations, rotations, points)"""
    def rel(got, want, ref0):
        nrm = np.linalg.norm(want - ref0, axis=1)
        err = np.linalg.norm(got - want, axis=1)
        moved = nrm[nrm > 0]
        floor = 0.01 * (np.median(moved) if len(moved) else 0.0)
        den = np.maximum(nrm, floor)
        return np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))
    q0 = prob["poses"][:, 3:] / np.linalg.norm(prob["poses"][:, 3:], axis=1, keepdims=True)
    q0 = np.where(q0[:, 3:4] < 0, -q0, q0)
    return (rel(got_poses[:, :3], want_poses[:, :3], prob["poses"][:, :3]),
            rel(got_poses[:, 3:], want_poses[:, 3:], q0),
            rel(got_points, want_points, prob["points"]))


def close_or_cascade(prob, got, want, want_perturbed=None, tol=TOL, tag=""):
    """got / want / want_perturbed: dicts with "poses" and "points".  Strict bar; if only points miss it and the reference's run from the
    perturbed input is given, the cascade-aware bar.  -> (worst relative error, cascaded?)"""
    t, r, p = block_errors(prob, got["poses"], got["points"], want["poses"], want["points"])
    worst_kf = max(float(t.max()), float(r.max()))
    assert worst_kf <= tol, (tag, "key frame block beyond %g: %.3g" % (tol, worst_kf))
    if float(p.max()) <= tol:
        return max(worst_kf, float(p.max())), False
    assert want_perturbed is not None, (tag, "%d points beyond %g, worst %.3g" % (int((p > tol).sum()), tol, float(p.max())))
    _, _, p_self = block_errors(prob, want_perturbed["poses"], want_perturbed["points"], want["poses"], want["points"])
    assert (p > tol).sum() <= 3 * (p_self > tol).sum() + 3 and p.max() <= 5 * max(float(p_self.max()), tol), (
        tag, "points beyond the bar %d (reference against itself: %d), worst %.3g (%.3g)" % ((p > tol).sum(), (p_self > tol).sum(), p.max(), p_self.max()))
    return float(p.max()), True


# ---- the references, computed once per process
@functools.lru_cache(maxsize=None)
def oracle_robust(name, its=ROBUST_ITS, perturb=False):
    """the oracle's robust one-stage optimisation (second stage of zero iterations), Huber(sqrt(5.991))"""
    prob = problem(name)
    return orc.ba_run(perturbed(prob) if perturb else prob, its=(its, 0))


@functools.lru_cache(maxsize=None)
def npref_run(name, robust, its, delta=npref.DELTA_GLOBAL, perturb=False):
    prob = problem(name)
    return npref.run(perturbed(prob) if perturb else prob, its, robust, delta)


def small_map():
    """One small map that exercises every rule of Optimizer::BundleAdjustment's collection (Optimizer.cpp:480-568): a bad key frame, a bad map
    point, an observation from a key frame that is missing from the list (mnId > maxKFid), a ray below cosFovTh, a point left without edges,
    all five faces, mnId == 0 not at index 0.  Plain arrays, the layout hm_global_ba_collect takes."""
    F = 650.0
    prob = synth.ba_problem(K=6, P=260, obs_per_point=4, F=int(F), seed=5)
    K, P = 6, 260
    rs = np.random.RandomState(7)
    # key frames of the list: indices 0..4 (ids 3, 0, 1, 2, 4: mnId == 0 at index 1); key frame 5 (id 9) is observed but NOT in the list
    kf_id = np.array([3, 0, 1, 2, 4, 9], np.int64)
    kf_bad = np.array([0, 0, 0, 1, 0, 0], np.uint8)
    nkp = 400
    keys = np.zeros((K, nkp, 2), np.float32); octave = np.zeros((K, nkp), np.int32); rays = np.zeros((K, nkp, 3), np.float32)
    rays[..., 2] = 1.0
    used = np.zeros(K, np.int64)
    obs_kf, obs_kp, obs_off = [], [], [0]
    order = np.argsort(prob["e_point"], kind="stable")
    face_seen = set()
    sig2 = (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2
    inv_tab = (np.float32(1.0) / sig2).astype(np.float32)
    for e in order:
        k = int(prob["e_pose"][e]); j = int(used[k]); used[k] += 1
        f = int(prob["e_face"][e]); face_seen.add(f)
        # cube-map pixel of the key point: face offsets as CamModelGeneral::FaceInCubemap cuts them (a 3F x 3F cross: up, left, front, right, down)
        ox, oy = {0: (1, 1), 1: (0, 1), 2: (2, 1), 3: (1, 0), 4: (1, 2)}[f]
        keys[k, j] = (np.float32(prob["e_obs"][e, 0] + ox * F), np.float32(prob["e_obs"][e, 1] + oy * F))
        octave[k, j] = int(np.argmin(np.abs(inv_tab.astype(np.float64) - prob["e_invsig2"][e])))
        rays[k, j] = (0.0, 0.0, 1.0)
        obs_kf.append(k); obs_kp.append(j)
    cnt = np.bincount(prob["e_point"], minlength=P)
    obs_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    obs_kf = np.array(obs_kf, np.int32); obs_kp = np.array(obs_kp, np.int32)
    mp_id = (np.arange(P) * 3 + 5).astype(np.int64)
    mp_bad = np.zeros(P, np.uint8); mp_bad[[7, 100]] = 1
    # rays below cosFovTh on a handful of observations; point 11 loses all of its edges that way
    low = rs.choice(len(obs_kf), 12, replace=False)
    for i in list(low) + list(range(obs_off[11], obs_off[12])):
        rays[obs_kf[i], obs_kp[i]] = (0.9, 0.0, -0.4)
    Tcw = np.zeros((K, 4, 4), np.float32)
    for k in range(K):
        x, y, z, w = prob["poses"][k, 3:] / np.linalg.norm(prob["poses"][k, 3:])
        Tcw[k, :3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        Tcw[k, :3, 3] = prob["poses"][k, :3]; Tcw[k, 3, 3] = 1
    assert sorted(face_seen) == [0, 1, 2, 3, 4]
    return dict(F=int(F), n_list=5, kf_id=kf_id, kf_bad=kf_bad, Tcw=Tcw, keys=keys, octave=octave, rays=rays, inv_level_sigma2=inv_tab,
                mp_id=mp_id, mp_bad=mp_bad, Xw=np.ascontiguousarray(prob["points"], np.float32), obs_off=obs_off, obs_kf=obs_kf, obs_kp=obs_kp,
                point_without_edges=11)
