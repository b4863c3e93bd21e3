"""ctypes access to the host build of the Initializer core (libcubemapslam_host.so: cubemapslam_amd/host/init_host.cpp) for the Initializer tests."""
import ctypes as C

import numpy as np

from cubemapslam_amd import api
from hostlib import load, p

_H = None
f32 = lambda a: np.ascontiguousarray(a, np.float32)


class Stages(C.Structure):
    """CmsInitStages (cubemapslam_amd/csrc/cms_init_core.h)"""
    _fields_ = [("A", C.c_float * 72), ("Vt", C.c_float * 81), ("W", C.c_double * 9), ("Epre", C.c_float * 9), ("w3", C.c_float * 3), ("u3", C.c_float * 9),
                ("vt3", C.c_float * 9)]


def H():
    global _H
    if _H is None:
        _H = load()
        _H.hm_init_cos_fov.argtypes = [C.c_double]; _H.hm_init_cos_fov.restype = C.c_float
        _H.hm_init_two_view_host.argtypes = [C.c_int, C.c_float, C.c_int, C.c_void_p]
        _H.hm_init_compute_e21.argtypes = [C.c_void_p] * 4
        _H.hm_init_check_essential.argtypes = [C.c_int, C.c_void_p, C.c_float, C.c_int] + [C.c_void_p] * 6; _H.hm_init_check_essential.restype = C.c_float
        _H.hm_init_check_rt.argtypes = [C.c_int, C.c_float] + [C.c_void_p] * 6
        _H.hm_init_decompose_e.argtypes = [C.c_void_p] * 4
        _H.hm_init_triangulate.argtypes = [C.c_void_p] * 7
        _H.hm_init_vector_sigma.argtypes = [C.c_int, C.c_float, C.c_float, C.c_void_p]; _H.hm_init_vector_sigma.restype = C.c_float
        _H.hm_init_decide.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _H.hm_init_resolve_draws.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        _H.hm_init_svd3.argtypes = [C.c_void_p] * 4
        assert _H.hm_init_stages_size() == C.sizeof(Stages)
    return _H


def cos_fov(camd):
    return float(H().hm_init_cos_fov(float(camd["fov_deg"])))


def two_view_host(F, cosfov, states):
    """hm_init_two_view_host over api.init_job_state() dicts -> (rc, results)"""
    arr = api.init_jobs(states)
    rc = H().hm_init_two_view_host(F, cosfov, len(states), arr)
    return rc, (api.init_results(arr, states) if rc == 0 else None)


def compute_e21(rays1, rays2):
    r1, r2 = f32(rays1), f32(rays2)
    E = np.zeros((3, 3), np.float32); st = Stages()
    H().hm_init_compute_e21(p(r1), p(r2), p(E), C.byref(st))
    g = lambda name, shape, t: np.array(getattr(st, name)[:], t).reshape(shape)
    return dict(E=E, A=g("A", (8, 9), np.float32), Vt=g("Vt", (9, 9), np.float32), W=g("W", 9, np.float64), Epre=g("Epre", (3, 3), np.float32),
                w3=g("w3", 3, np.float32), u3=g("u3", (3, 3), np.float32), vt3=g("vt3", (3, 3), np.float32))


def check_essential(F, E, sigma, rays1, rays2, keys1, keys2):
    N = len(rays1)
    inl = np.zeros(N, np.uint8); terms = np.zeros((N, 2), np.float32)
    E = f32(E); a = [f32(rays1), f32(rays2), f32(keys1), f32(keys2)]
    score = H().hm_init_check_essential(F, p(E), float(sigma), N, *[p(v) for v in a], p(inl), p(terms))
    return np.float32(score), inl.astype(bool), terms


def check_rt(F, cosfov, state, R, t):
    arr = api.init_jobs([state])
    n1 = state["n1"]
    P = np.zeros((n1, 3), np.float32); good = np.zeros(n1, np.uint8); c = C.c_float()
    R = f32(R); t = f32(t)
    n = H().hm_init_check_rt(F, cosfov, arr, p(R), p(t), p(P), p(good), C.byref(c))
    assert n >= 0
    return n, P, good.astype(bool), np.float32(c.value)


def decompose_e(E):
    E = f32(E); R1 = np.zeros((3, 3), np.float32); R2 = np.zeros((3, 3), np.float32); t = np.zeros(3, np.float32)
    H().hm_init_decompose_e(p(E), p(R1), p(R2), p(t))
    return R1, R2, t


def triangulate(ray1, ray2, Ra, ta, Rb, tb):
    a = [f32(v) for v in (ray1, ray2, Ra, ta, Rb, tb)]
    x = np.zeros(3, np.float32)
    H().hm_init_triangulate(*[p(v) for v in a], p(x))
    return x


def vector_sigma(F, kx, ky, n):
    n = f32(n)
    return np.float32(H().hm_init_vector_sigma(F, float(kx), float(ky), p(n)))


def decide(nGood, cosines, N):
    g = np.ascontiguousarray(nGood, np.int32); c = f32(cosines); par = np.zeros(4, np.float32)
    w = H().hm_init_decide(p(g), p(c), int(N), p(par))
    return w, par


def resolve_draws(N, row):
    r = np.ascontiguousarray(row, np.int32); idx = np.zeros(8, np.int32)
    H().hm_init_resolve_draws(N, p(r), p(idx))
    return idx


def svd3(A):
    A = f32(A); w = np.zeros(3, np.float32); u = np.zeros((3, 3), np.float32); vt = np.zeros((3, 3), np.float32)
    H().hm_init_svd3(p(A), p(w), p(u), p(vt))
    return w, u, vt


def mirror(engine, camd, pr, sigma, iterations, draws, p3d_before=None, tri_before=None):
    """class Initializer of cubemap_hot_path.h through hm_init_mirror on a problem of init_cases; engine 1 = the host build of the core, 0 = the device.
    draws None: the class draws for itself.
    p3d_before / tri_before: what vP3D and vbTriangulated hold when InitializeWithRays is called."""
    L = H()
    L.hm_last_error.restype = C.c_char_p
    assert L.hm_set_camera(C.byref(api.make_camera(camd))) == 0, L.hm_last_error()
    n1, n2 = len(pr["keys1"]), len(pr["keys2"])
    k1 = np.zeros(n1, api.KP_DTYPE); k1["x"] = pr["keys1"][:, 0]; k1["y"] = pr["keys1"][:, 1]
    k2 = np.zeros(n2, api.KP_DTYPE); k2["x"] = pr["keys2"][:, 0]; k2["y"] = pr["keys2"][:, 1]
    r1, r2 = f32(pr["rays1"]), f32(pr["rays2"]); m = np.ascontiguousarray(pr["matches12"], np.int32)
    default_draw = draws is None                                    # the class's own draw: srand(0) once per process, RandomInt's formula
    dr = np.zeros(1, np.int32) if default_draw else np.ascontiguousarray(draws, np.int32).ravel()
    p3d_before = np.zeros((0, 3), np.float32) if p3d_before is None else f32(p3d_before)
    tri_before = np.zeros(0, np.uint8) if tri_before is None else np.ascontiguousarray(tri_before, np.uint8)
    p3d = np.zeros((max(n1, len(p3d_before), 1), 3), np.float32); p3d[:len(p3d_before)] = p3d_before
    tri = np.zeros(max(n1, len(tri_before), 1), np.uint8); tri[:len(tri_before)] = tri_before
    R = np.zeros(9, np.float32); t = np.zeros(3, np.float32); sets = np.full(8 * iterations, -1, np.int32); state = np.zeros(12, np.int32); diag = np.zeros(5, np.float32)
    L.hm_init_mirror.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = L.hm_init_mirror(engine, n1, p(k1), p(r1), n2, p(k2), p(r2), p(m), float(sigma), int(iterations), -1 if default_draw else len(dr), p(dr), p(R), p(t), len(p3d_before), p(p3d),
                          len(tri_before), p(tri), p(sets), p(state), p(diag))
    assert rc == 0, L.hm_last_error()
    return dict(found=int(state[0]), draws_used=int(state[1]), N=int(state[2]), R21=R, t21=t, p3d=p3d[:state[3]].copy(), triangulated=tri[:state[4]].copy(),
                sets=sets.reshape(iterations, 8), best_iteration=int(state[5]), n_inliers=int(state[6]), winner=int(state[7]), nGood=state[8:12].copy(),
                score=diag[:1].copy(), parallax=diag[1:5].copy())
