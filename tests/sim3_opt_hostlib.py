"""ctypes access to the host build of the OptimizeSim3 core (libcubemapslam_host.so: cubemapslam_amd/host/sim3_opt_host.cpp) for the tests."""
import ctypes as C

import numpy as np

from cubemapslam_amd import api
from hostlib import load, p

_H = None
V = C.c_void_p


def H():
    global _H
    if _H is None:
        _H = load()
        _H.hm_sim3_optimize_host.argtypes = [C.c_int, C.c_int, V]
        _H.hm_sim3_opt_last_reason.restype = C.c_char_p
        _H.hm_s3o_exp.argtypes = [C.c_double]; _H.hm_s3o_exp.restype = C.c_double
        _H.hm_s3o_sincos.argtypes = [C.c_double, V, V]; _H.hm_s3o_sincos.restype = None
        _H.hm_s3o_sim3_exp.argtypes = [V, V]; _H.hm_s3o_sim3_exp.restype = None
        _H.hm_s3o_R_to_quat.argtypes = [V, V]; _H.hm_s3o_R_to_quat.restype = None
        _H.hm_s3o_oplus.argtypes = [V, V, C.c_int, V]; _H.hm_s3o_oplus.restype = None
        _H.hm_s3o_inverse.argtypes = [V, V]; _H.hm_s3o_inverse.restype = None
        _H.hm_s3o_edge_errors.argtypes = [C.c_int] + [V] * 6
        _H.hm_s3o_edge_jacobians.argtypes = [C.c_int, C.c_int, C.c_int] + [V] * 7
        _H.hm_s3o_solve7.argtypes = [V, V, C.c_double, V]
        _H.hm_s3o_tree.argtypes = [V]; _H.hm_s3o_tree.restype = C.c_double
    return _H


def optimize_host(F, states):
    """hm_sim3_optimize_host over api.sim3_opt_job_state() dicts -> (rc, results)"""
    arr = api.sim3_opt_jobs(states)
    rc = H().hm_sim3_optimize_host(F, len(states), arr)
    return rc, (api.sim3_opt_results(arr, states) if rc == 0 else None)


def det_exp(x):
    return H().hm_s3o_exp(float(x))


def det_sincos(x):
    s = C.c_double(); c = C.c_double()
    H().hm_s3o_sincos(float(x), C.byref(s), C.byref(c))
    return s.value, c.value


# the core's own exp / sin / cos for npref_sim3_opt's injectable callables
FN = dict(exp=det_exp, sin=lambda x: det_sincos(x)[0], cos=lambda x: det_sincos(x)[1])


def _s8(S):
    return np.ascontiguousarray(np.concatenate([np.asarray(S[0], np.float64), np.asarray(S[1], np.float64), [float(S[2])]]))


def _from8(o):
    return o[:4].copy(), o[4:7].copy(), np.float64(o[7])


def sim3_exp(u):
    u = np.ascontiguousarray(u, np.float64); o = np.zeros(8)
    H().hm_s3o_sim3_exp(p(u), p(o))
    return _from8(o)


def R_to_quat(R):
    R = np.ascontiguousarray(R, np.float64); q = np.zeros(4)
    H().hm_s3o_R_to_quat(p(R), p(q))
    return q


def oplus(S, u, fix_scale):
    u = np.ascontiguousarray(u, np.float64).copy(); o = np.zeros(8); s8 = _s8(S)
    H().hm_s3o_oplus(p(s8), p(u), int(fix_scale), p(o))
    return _from8(o), u


def inverse(S):
    o = np.zeros(8); s8 = _s8(S)
    H().hm_s3o_inverse(p(s8), p(o))
    return _from8(o)


def _pair(case, k):
    return [np.ascontiguousarray(case[n][k], np.float32) for n in ("x3dc1", "x3dc2", "kp1", "kp2")]


def edge_errors(F, S, case, k):
    """(e12, e21) of correspondence k of a case at S"""
    a = _pair(case, k); e = np.zeros(4); s8 = _s8(S)
    assert H().hm_s3o_edge_errors(F, p(s8), *[p(v) for v in a], p(e)) == 0
    return e[:2].copy(), e[2:].copy()


def edge_jacobians(F, mode, fix_scale, S, case, k):
    """(J12, J21), 2 x 7 each, of correspondence k of a case at S"""
    a = _pair(case, k); J12 = np.zeros((2, 7)); J21 = np.zeros((2, 7)); s8 = _s8(S)
    assert H().hm_s3o_edge_jacobians(F, int(mode), int(fix_scale), p(s8), *[p(v) for v in a], p(J12), p(J21)) == 0
    return J12, J21


def solve7(Hm, b, lam):
    Hm = np.ascontiguousarray(Hm, np.float64); b = np.ascontiguousarray(b, np.float64); x = np.zeros(7)
    ok = H().hm_s3o_solve7(p(Hm), p(b), float(lam), p(x))
    return bool(ok), x


def tree(slots):
    s = np.ascontiguousarray(slots, np.float64)
    assert s.shape == (H().hm_s3o_slots(),)
    return H().hm_s3o_tree(p(s))


def mirror_case(seed=21, N=90, fix_scale=False):
    """sim3_hostlib.mirror_case (holes, bad points, points without an index; its points behind every face and its random outliers made consistent, see below) with what Optimizer::OptimizeSim3 reads on top:
    key points (the float projection of the key point's own map point plus half a pixel of noise, where there is one in a face; elsewhere a point
    inside some face), mvInvLevelSigma2, and the start S12 = the case's true similarity a little off.  Returns (camd, kf1, kf2, m12, start)."""
    import sim3_cases
    import sim3_hostlib
    import sim3_opt_cases as oc
    from npref_pnp import rays_to_cubemap
    from cubemapslam_amd import synth
    camd, kf1, kf2, m12, _ = sim3_hostlib.mirror_case(seed, N, fix_scale)
    pr = sim3_cases.problem(seed, N=N, outliers=0.3, fix_scale=int(fix_scale))      # the problem mirror_case built its key frames from
    rng = np.random.default_rng(seed + 500)
    F = oc.F
    # the problem's outliers are random points of key frame 2; mapped into key frame 1 many of them fall behind the face of their key point, where the
    # projection is wild and (as in the reference) nothing survives the first round.  They get the consistent point back; the gross outliers of this
    # case are made in the image instead, below
    T2 = kf2["Tcw"].astype(np.float64)
    for j in np.nonzero(pr["outlier"])[0]:
        X2 = pr["s21"] * pr["R21"] @ pr["x3dc1"][j].astype(np.float64) + pr["t21"]
        kf2["pos"][kf2["slot"][j]] = ((X2 - T2[:, 3]) @ T2[:, :3]).astype(np.float32)
    # OptimizeSim3 has no projection filter: a point behind every face would stay in the graph with a residual of thousands of pixels and a Jacobian to
    # match.  mirror_case's points behind the faces get the position their partner implies
    T1 = kf1["Tcw"].astype(np.float64)
    for i in range(len(m12)):
        if m12[i] < 0 or kf1["mp"][i] < 0:
            continue
        s1, s2 = kf1["mp"][i], m12[i]
        X1 = sim3_hostlib.camera_points(kf1["Tcw"], kf1["pos"][s1:s1 + 1])[0].astype(np.float64)
        X2 = sim3_hostlib.camera_points(kf2["Tcw"], kf2["pos"][s2:s2 + 1])[0].astype(np.float64)
        if not sim3_cases.in_a_face(X1[None])[0]:
            X1 = pr["s12"] * pr["R12"] @ X2 + pr["t12"]
            kf1["pos"][s1] = ((X1 - T1[:, 3]) @ T1[:, :3]).astype(np.float32)
        if not sim3_cases.in_a_face(X2[None])[0]:
            X2 = pr["s21"] * pr["R21"] @ X1 + pr["t21"]
            kf2["pos"][s2] = ((X2 - T2[:, 3]) @ T2[:, :3]).astype(np.float32)
    for kf in (kf1, kf2):
        nk = len(kf["octave"])
        origin = np.array([(1, 1), (0, 1), (2, 1), (1, 0), (1, 2)], np.float64)[rng.integers(0, 5, nk)] * F
        kp = (origin + rng.uniform(4, F - 4, (nk, 2))).astype(np.float32)
        Xc = sim3_hostlib.camera_points(kf["Tcw"], kf["pos"])
        _, u, v = rays_to_cubemap(F, Xc[:, 0], Xc[:, 1], Xc[:, 2])
        where = kf["mp"] if "mp" in kf else None
        for slot in range(len(kf["pos"])):
            # key frame 1: the key point that HOLDS the map point (GetMapPointMatches); key frame 2: the key point the map point names (GetIndexInKeyFrame)
            ks = np.nonzero(where == slot)[0] if where is not None else ([kf["index_in_kf"][slot]] if kf["index_in_kf"][slot] >= 0 else [])
            for k in ks:
                if u[slot] >= 0 and v[slot] >= 0:
                    o = np.floor(np.array([u[slot], v[slot]], np.float64) / F) * F
                    kp[k] = np.clip(np.array([u[slot], v[slot]]) + rng.normal(0, 0.5, 2), o + 0.5, o + F - 0.5).astype(np.float32)
        gross = rng.uniform(size=nk) < 0.2      # a fifth of the key points 30 - 120 pixels off, inside their face
        ang = rng.uniform(0, 2 * np.pi, nk); rad = rng.uniform(30, 120, nk)
        o = np.floor(kp.astype(np.float64) / F) * F
        moved = np.clip(kp + np.stack([np.cos(ang), np.sin(ang)], 1) * rad[:, None], o + 0.5, o + F - 0.5).astype(np.float32)
        kp[gross] = moved[gross]
        kf["kpts"] = kp
        kf["inv_sigma2"] = (np.float32(1.0) / np.asarray(kf["sigma2"], np.float32)).astype(np.float32)
    dR = synth._rot(rng.normal(size=3), np.deg2rad(0.3))
    start = dict(R12=dR @ pr["R12"], t12=pr["t12"] + 0.01 * rng.normal(size=3) / np.sqrt(3), s12=float(pr["s12"]) * (1.0 if fix_scale else 1.01))
    return camd, kf1, kf2, m12, start


def mirror_expected_graph(kf1, kf2, m12):
    """The job arrays Optimizer.cpp:941-1028 makes: per key point i of key frame 1 with vpMatches1[i], an own map point, neither point bad and
    GetIndexInKeyFrame(pKF2) >= 0 -- no test of key frame 1's index, none of the projection -- P3D1c | P3D2c, both key points' pt, both invSigma2"""
    import sim3_hostlib
    m12 = np.asarray(m12)
    idx = np.array([i for i in range(len(m12)) if m12[i] >= 0 and kf1["mp"][i] >= 0 and not kf1["bad"][kf1["mp"][i]] and not kf2["bad"][m12[i]]
                    and kf2["index_in_kf"][m12[i]] >= 0], np.int32)
    s1 = kf1["mp"][idx]; s2 = m12[idx]; i2 = kf2["index_in_kf"][s2]
    return dict(idx=idx, x3dc1=sim3_hostlib.camera_points(kf1["Tcw"], kf1["pos"][s1]), x3dc2=sim3_hostlib.camera_points(kf2["Tcw"], kf2["pos"][s2]),
                kp1=kf1["kpts"][idx], kp2=kf2["kpts"][i2], inv_sigma2_1=kf1["inv_sigma2"][kf1["octave"][idx]], inv_sigma2_2=kf2["inv_sigma2"][kf2["octave"][i2]])


def mirror(engine, camd, kf1, kf2, m12, start, th2, fix_scale, jacobian=0):
    """Optimizer::OptimizeSim3 of cubemap_hot_path.h through hm_sim3_opt_mirror.  engine 1 = the host build of the core, 0 = the device.
    -> dict(N, idx, x3dc1, x3dc2, kp1, kp2, inv_sigma2_1, inv_sigma2_2 (what the call made of the graph), matches1 (vpMatches1 afterwards), n_inliers, q12, t12, s12)"""
    L = H()
    assert L.hm_set_camera(C.byref(api.make_camera(camd))) == 0, L.hm_last_error()
    n1 = len(m12)
    arrs = []
    for kf in (kf1, kf2):
        arrs += [np.ascontiguousarray(kf["Tcw"], np.float32), np.ascontiguousarray(kf["inv_sigma2"], np.float32), np.ascontiguousarray(kf["octave"], np.int32),
                 np.ascontiguousarray(kf["kpts"], np.float32), np.ascontiguousarray(kf["pos"], np.float32), np.ascontiguousarray(kf["bad"], np.uint8),
                 np.ascontiguousarray(kf["index_in_kf"], np.int32)]
    mp1 = np.ascontiguousarray(kf1["mp"], np.int32); m = np.array(m12, np.int32).copy()
    S12 = np.concatenate([np.asarray(start["R12"], np.float64).ravel(), np.asarray(start["t12"], np.float64), [float(start["s12"])]])
    N = C.c_int(); nin = C.c_int(); cap = max(n1, 1)
    idx = np.zeros(cap, np.int32); x12 = np.zeros((cap, 6), np.float32); kp12 = np.zeros((cap, 4), np.float32); is12 = np.zeros((cap, 2), np.float32); out8 = np.zeros(8)
    L.hm_sim3_opt_mirror.argtypes = [C.c_int] * 8 + [V] * 17 + [C.c_float, C.c_int] + [V] * 7
    rc = L.hm_sim3_opt_mirror(int(engine), int(jacobian), n1, len(kf1["octave"]), len(kf2["octave"]), len(kf1["inv_sigma2"]), len(kf1["bad"]), len(kf2["bad"]),
                              *[p(a) for a in arrs], p(mp1), p(m), p(S12), float(th2), 1 if fix_scale else 0, C.byref(N), p(idx), p(x12), p(kp12), p(is12), p(out8), C.byref(nin))
    assert rc == 0, L.hm_last_error()
    n = N.value
    return dict(N=n, idx=idx[:n].copy(), x3dc1=x12[:n, :3].copy(), x3dc2=x12[:n, 3:].copy(), kp1=kp12[:n, :2].copy(), kp2=kp12[:n, 2:].copy(),
                inv_sigma2_1=is12[:n, 0].copy(), inv_sigma2_2=is12[:n, 1].copy(), matches1=m, n_inliers=nin.value, q12=out8[:4].copy(), t12=out8[4:7].copy(), s12=out8[7:8].copy())
