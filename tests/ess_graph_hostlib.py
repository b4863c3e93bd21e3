"""ctypes access to the host build of the OptimizeEssentialGraph core (libcubemapslam_host.so: cubemapslam_amd/host/ess_graph_host.cpp) for the tests."""
import ctypes as C

import numpy as np

import sim3_opt_hostlib
from cubemapslam_amd import api
from hostlib import load, p

_H = None
V = C.c_void_p


def H():
    global _H
    if _H is None:
        _H = load()
        _H.hm_essential_graph_optimize_host.argtypes = [C.c_int, V]
        _H.hm_ess_graph_job_check.argtypes = [C.c_int, V] + [C.c_int] * 4
        _H.hm_ess_graph_last_reason.restype = C.c_char_p
        _H.hm_sim3_correct_points_host.argtypes = [C.c_int, V, V, C.c_int, V, V, V]
        _H.hm_det_log.argtypes = [C.c_double]; _H.hm_det_log.restype = C.c_double
        _H.hm_det_acos.argtypes = [C.c_double]; _H.hm_det_acos.restype = C.c_double
        _H.hm_eg_log.argtypes = [V, V]; _H.hm_eg_log.restype = None
        _H.hm_eg_edge_error.argtypes = [V] * 5; _H.hm_eg_edge_error.restype = None
        _H.hm_eg_edge_jacobians.argtypes = [V] * 4 + [C.c_int, V, V]; _H.hm_eg_edge_jacobians.restype = None
        _H.hm_eg_envelope.argtypes = [C.c_int, C.c_int, C.c_int, V, V]; _H.hm_eg_envelope.restype = C.c_longlong
        _H.hm_eg_envelope_solve.argtypes = [C.c_int, C.c_int, C.c_int, V, V, V, C.c_double, V]
    return _H


def reason():
    return H().hm_ess_graph_last_reason().decode()


def optimize_host(states):
    """hm_essential_graph_optimize_host over api.ess_graph_job_state() dicts -> (rc, results)"""
    arr = api.ess_graph_jobs(states)
    rc = H().hm_essential_graph_optimize_host(len(states), arr)
    return rc, (api.ess_graph_results(arr, states) if rc == 0 else None)


def job_check(states, max_jobs=64, max_vertices=1 << 20, max_edges=1 << 20, max_blocks=1 << 24, arr=None):
    """hm_ess_graph_job_check -> (rc, reason, the job array)"""
    arr = api.ess_graph_jobs(states) if arr is None else arr
    rc = H().hm_ess_graph_job_check(len(states), arr, max_jobs, max_vertices, max_edges, max_blocks)
    return rc, reason(), arr


det_log = lambda x: H().hm_det_log(float(x))
det_acos = lambda x: H().hm_det_acos(float(x))
# the core's own elementary functions for the restatement's injectable callables
FN = dict(sim3_opt_hostlib.FN, log=det_log, acos=det_acos)


def _r8(S):
    return np.ascontiguousarray(np.concatenate([np.asarray(S[0], np.float64), np.asarray(S[1], np.float64), [float(S[2])]]))


def eg_log(S):
    s8 = _r8(S); u = np.zeros(7)
    H().hm_eg_log(p(s8), p(u))
    return u


def edge_error(Mi, Mj, S0, S1):
    a = [_r8(x) for x in (Mi, Mj, S0, S1)]; e = np.zeros(7)
    H().hm_eg_edge_error(*[p(x) for x in a], p(e))
    return e


def edge_jacobians(Mi, Mj, S0, S1, fix_scale):
    a = [_r8(x) for x in (Mi, Mj, S0, S1)]; J0 = np.zeros((7, 7)); J1 = np.zeros((7, 7))
    H().hm_eg_edge_jacobians(*[p(x) for x in a], int(fix_scale), p(J0), p(J1))
    return J0, J1


def envelope(N, fixed, edges):
    """-> (first, block count)"""
    e = np.ascontiguousarray(edges, np.int32).reshape(-1, 3); first = np.zeros(max(N - 1, 1), np.int32)
    B = H().hm_eg_envelope(N, fixed, len(e), p(e), p(first))
    return first[:N - 1].copy(), int(B)


def envelope_solve(N, fixed, edges, Hd, b, lam):
    e = np.ascontiguousarray(edges, np.int32).reshape(-1, 3)
    Hd = np.ascontiguousarray(Hd, np.float64); b = np.ascontiguousarray(b, np.float64); x = np.zeros(len(b))
    ok = H().hm_eg_envelope_solve(N, fixed, len(e), p(e), p(Hd), p(b), float(lam), p(x))
    return bool(ok), x


def correct_points_host(pos, ref, S_old, S_new):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); ref = np.ascontiguousarray(ref, np.int32)
    S_old = np.ascontiguousarray(S_old, np.float64); S_new = np.ascontiguousarray(S_new, np.float64)
    out = np.full((max(len(pos), 1), 3), 7.0, np.float32)
    rc = H().hm_sim3_correct_points_host(len(pos), p(pos), p(ref), len(S_old), p(S_old), p(S_new), p(out))
    assert rc == 0, reason()
    return out[:len(pos)]


def mirror(engine, m):
    """Optimizer::OptimizeEssentialGraph of cubemap_hot_path.h through hm_ess_graph_mirror on an ess_graph_cases.mirror_case().  engine 1 = the host build
    of the core, 0 = the device.  -> dict(vertex_kf, edges, fixed (what CollectEssentialGraph made), Tcw, mp_pos (what the call wrote back))"""
    L = H()
    from cubemapslam_amd import synth
    assert L.hm_set_camera(C.byref(api.make_camera(synth.camera("lafida", 150)))) == 0, L.hm_last_error()      # the shared context of the device engine wants one
    kfs = m["kfs"]; nkf = len(kfs)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)

    def csr(lists):
        off = np.zeros(len(lists) + 1, np.int32); off[1:] = np.cumsum([len(x) for x in lists])
        return off, i32([v for x in lists for v in x] + [0])
    child_off, child = csr([sorted(k["children"]) for k in kfs]); loop_off, loop = csr([sorted(k["loop_edges"]) for k in kfs])
    cov_off, cov = csr([k["cov"] for k in kfs]); _, cov_w = csr([k["cov_w"] for k in kfs])
    Tcw = np.ascontiguousarray(np.stack([k["Tcw"] for k in kfs]), np.float32).copy()
    mp_pos = np.ascontiguousarray(m["mp_pos"], np.float32).copy()
    poses = lambda d: (i32(sorted(d)), np.ascontiguousarray(np.stack([d[k] for k in sorted(d)]), np.float64))
    nc_kf, nc_S = poses(m["non_corrected"]); c_kf, c_S = poses(m["corrected"])
    lc_keys = sorted(m["loop_connections"]); lc_off, lc = csr([sorted(m["loop_connections"][k]) for k in lc_keys])
    cap_v, cap_e = nkf, 8 * nkf
    N = C.c_int(); E = C.c_int(); fixed = C.c_int(); vertex_kf = np.zeros(cap_v, np.int32); edges = np.zeros((cap_e, 3), np.int32)
    L.hm_ess_graph_mirror.argtypes = [C.c_int, C.c_int] + [V] * 11 + [C.c_int] + [V] * 5 + [C.c_int, C.c_int, C.c_int, V, V, C.c_int, V, V, C.c_int, V, V, V, C.c_int, C.c_int, C.c_int] + [V] * 5
    rc = L.hm_ess_graph_mirror(int(engine), nkf, p(i32([k["mnId"] for k in kfs])), p(np.array([k["bad"] for k in kfs], np.uint8)), p(Tcw), p(i32([k["parent"] for k in kfs])),
                               p(child_off), p(child), p(loop_off), p(loop), p(cov_off), p(cov), p(cov_w), len(mp_pos), p(np.ascontiguousarray(m["mp_bad"], np.uint8)), p(mp_pos),
                               p(i32(m["mp_ref"])), p(i32(m["mp_by"])), p(i32(m["mp_cref"])), int(m["loop"]), int(m["cur"]), len(nc_kf), p(nc_kf), p(nc_S), len(c_kf), p(c_kf),
                               p(c_S), len(lc_keys), p(i32(lc_keys)), p(lc_off), p(lc), int(m["fix_scale"]), cap_v, cap_e, C.byref(N), C.byref(E), p(vertex_kf), p(edges),
                               C.byref(fixed))
    assert rc == 0, L.hm_last_error()
    return dict(vertex_kf=vertex_kf[:N.value].copy(), edges=edges[:E.value].copy(), fixed=fixed.value, Tcw=Tcw, mp_pos=mp_pos)
