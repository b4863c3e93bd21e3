"""ctypes access to the host build of the PnP core (libcubemapslam_host.so: cubemapslam_amd/host/pnp_host.cpp) for the PnP tests."""
import ctypes as C

import numpy as np

from cubemapslam_amd import api
from hostlib import load, p

_H = None


class Stages(C.Structure):
    """CmsPnpStages (cubemapslam_amd/csrc/cms_pnp_core.h)"""
    _fields_ = [("cws", C.c_double * 12), ("dc", C.c_double * 3), ("uct", C.c_double * 9), ("d", C.c_double * 12), ("l_6x10", C.c_double * 60),
                ("rho", C.c_double * 6), ("betas0", C.c_double * 12), ("betas", C.c_double * 12), ("Rs", C.c_double * 27), ("ts", C.c_double * 9),
                ("rep", C.c_double * 3), ("chosen", C.c_int)]


def H():
    global _H
    if _H is None:
        _H = load()
        _H.hm_pnp_iterate_host.argtypes = [C.c_int, C.c_int, C.c_void_p]
        _H.hm_pnp_compute_pose.argtypes = [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        _H.hm_pnp_check_inliers.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6
        _H.hm_pnp_jacobi.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3
        _H.hm_pnp_resolve_draws.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        assert _H.hm_pnp_stages_size() == C.sizeof(Stages)
    return _H


def iterate_host(F, states):
    """hm_pnp_iterate_host over api.pnp_job_state() dicts -> (rc, results)"""
    arr = api.pnp_jobs(states)
    rc = H().hm_pnp_iterate_host(F, len(states), arr)
    return rc, (api.pnp_results(arr, states) if rc == 0 else None)


def compute_pose(F, state, idx):
    """One EPnP solve of the core on correspondences idx of a job state -> dict of every stage"""
    arr = api.pnp_jobs([state])
    idx = np.ascontiguousarray(idx, np.int32)
    n = len(idx)
    st = Stages(); ut = np.zeros((12, 12)); al = np.zeros((n, 4)); R = np.zeros((3, 3)); t = np.zeros(3); rep = C.c_double()
    rc = H().hm_pnp_compute_pose(F, arr, n, p(idx), C.byref(st), p(ut), p(al), p(R), p(t), C.byref(rep))
    assert rc == 0, rc
    g = lambda name, shape: np.array(getattr(st, name)[:]).reshape(shape)
    return dict(cws=g("cws", (4, 3)), dc=g("dc", 3), uct=g("uct", (3, 3)), d=g("d", 12), ut=ut, alphas=al, L=g("l_6x10", (6, 10)), rho=g("rho", 6),
                betas0=g("betas0", (3, 4)), betas=g("betas", (3, 4)), Rs=g("Rs", (3, 3, 3)), ts=g("ts", (3, 3)), rep=g("rep", 3), chosen=st.chosen, R=R, t=t,
                rep_error=rep.value, pws=state["p3d"][idx].astype(np.float64), us=state["p2d"][idx].astype(np.float64),
                bearings=state["bearing"][idx].astype(np.float64))


def jacobi(A):
    """The core's SVD of A (m x n) -> (AV rows = w_k u_k, w, Vt)"""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    At = np.ascontiguousarray(A.T); Vt = np.zeros((n, n)); w = np.zeros(n)
    H().hm_pnp_jacobi(m, n, p(At), p(Vt), p(w))
    return At, w, Vt


def check_inliers(F, R, t, p3d, p2d, max_error):
    out = np.zeros(len(p3d), np.uint8)
    R = np.ascontiguousarray(R, np.float64); t = np.ascontiguousarray(t, np.float64)
    p3d = np.ascontiguousarray(p3d, np.float32); p2d = np.ascontiguousarray(p2d, np.float32); max_error = np.ascontiguousarray(max_error, np.float32)
    c = H().hm_pnp_check_inliers(F, len(p3d), p(R), p(t), p(p3d), p(p2d), p(max_error), p(out))
    assert c == int(out.sum())
    return out.astype(bool)


def mirror(engine, camd, frame, mp, bad, pos, n_iterations, draws, probability=0.99, min_inliers=8, max_iterations=300, epsilon=0.4, th2=5.991):
    """class PnPsolver of cubemap_hot_path.h through hm_pnp_mirror: frame = dict(kps (api.KP_DTYPE), rays (n x 3), sigma2 (levels)); mp / bad / pos per key
    point; one iterate() per entry of n_iterations until a pose or bNoMore.  engine 1 = the host build of the core, 0 = the device."""
    L = H()
    L.hm_last_error.restype = C.c_char_p
    assert L.hm_set_camera(C.byref(api.make_camera(camd))) == 0, L.hm_last_error()
    n = len(frame["kps"])
    kps = np.ascontiguousarray(frame["kps"]); rays = np.ascontiguousarray(frame["rays"], np.float32); mp = np.ascontiguousarray(mp, np.int64)
    bad = np.ascontiguousarray(bad, np.uint8); pos = np.ascontiguousarray(pos, np.float32); sg = np.ascontiguousarray(frame["sigma2"], np.float32)
    its = np.ascontiguousarray(n_iterations, np.int32); dr = np.ascontiguousarray(draws, np.int32).ravel()
    N = C.c_int(); key_idx = np.zeros(max(n, 1), np.int32); vb = np.zeros(max(n, 1), np.uint8); T = np.zeros(16, np.float32); state = np.zeros(5, np.int32)
    L.hm_pnp_mirror.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    rc = L.hm_pnp_mirror(engine, n, p(kps), p(rays), p(mp), p(bad), p(pos), len(sg), p(sg), probability, min_inliers, max_iterations, epsilon, th2, len(its), p(its),
                         len(dr), p(dr), C.byref(N), p(key_idx), p(vb), p(T), p(state))
    assert rc == 0, L.hm_last_error()
    return dict(N=N.value, key_idx=key_idx[:N.value].copy(), vbInliers=vb[:n].copy(), Tcw=T.reshape(4, 4).copy(), no_more=int(state[0]), n_inliers=int(state[1]),
                iterations=int(state[2]), found=int(state[3]), draws_used=int(state[4]))


def mirror_case(seed=21, N=70):
    """A frame of n key points of which some hold no map point (-1) and some a bad one, for the mirror class: returns (camd, frame, mp, bad, pos, kept),
    kept = the key points PnPsolver's constructor keeps, in order, with the job arrays they make"""
    import pnp_cases as pc
    from cubemapslam_amd import synth
    pr = pc.problem(seed, N=N, outliers=0.25, noise=0.8)
    rng = np.random.default_rng(seed)
    n = N + 25
    where = np.sort(rng.choice(n, N, replace=False))                  # key points that hold the problem's correspondences
    kps = np.zeros(n, api.KP_DTYPE); kps["x"] = rng.uniform(0, 3 * pc.F, n); kps["y"] = rng.uniform(0, 3 * pc.F, n); kps["octave"] = rng.integers(0, 8, n)
    rays = rng.normal(size=(n, 3)).astype(np.float32); pos = rng.normal(size=(n, 3)).astype(np.float32)
    kps["x"][where] = pr["p2d"][:, 0]; kps["y"][where] = pr["p2d"][:, 1]; rays[where] = pr["bearing"]; pos[where] = pr["p3d"]
    sigma2 = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    mp = np.full(n, -1, np.int64); mp[where] = 1000 + np.arange(N)
    bad = np.zeros(n, np.uint8); bad_at = rng.choice(where, 9, replace=False); bad[bad_at] = 1
    stray = np.setdiff1d(np.arange(n), where)[:4]; bad[stray] = 1         # bad flags on key points without a map point change nothing
    kept = np.array([i for i in where if not bad[i]], np.int32)
    job = dict(p3d=pos[kept], p2d=np.stack([kps["x"][kept], kps["y"][kept]], 1), bearing=rays[kept], sigma2=sigma2[kps["octave"][kept]])
    return synth.camera("lafida", pc.F), dict(kps=kps, rays=rays, sigma2=sigma2), mp, bad, pos, kept, job
