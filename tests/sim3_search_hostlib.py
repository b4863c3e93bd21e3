"""ctypes access to the host build of the SearchBySim3 core and job check (libcubemapslam_host.so: cubemapslam_amd/host/sim3_search_host.cpp)."""
import ctypes as C

import numpy as np

from hostlib import load, p

_H = None


class Job(C.Structure):
    """cms_sim3_search_job (include/cubemapslam_hip.h)"""
    _fields_ = [("slot1", C.c_int), ("n1", C.c_int), ("slot2", C.c_int), ("n2", C.c_int), ("s12", C.c_float), ("R12", C.c_float * 9), ("t12", C.c_float * 3),
                ("off1", C.c_int), ("off2", C.c_int)]


def H():
    global _H
    if _H is None:
        _H = load()
        _H.hm_sim3s_compose.argtypes = [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        _H.hm_sim3s_compose.restype = None
        _H.hm_sim3s_project.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
        _H.hm_sim3s_project.restype = None
        _H.hm_sim3s_job_check.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_char_p, C.c_int]
        assert _H.hm_sim3s_motion_size() == 24 * 4
    return _H


def compose(s12, R12, t12):
    """cms_sim3s_compose -> dict(sR12, t12, sR21, t21)"""
    R = np.ascontiguousarray(R12, np.float32).reshape(9); t = np.ascontiguousarray(t12, np.float32).reshape(3)
    out = np.zeros(24, np.float32)
    H().hm_sim3s_compose(float(np.float32(s12)), p(R), p(t), p(out))
    return dict(sR12=out[:9].reshape(3, 3).copy(), t12=out[9:12].copy(), sR21=out[12:21].reshape(3, 3).copy(), t21=out[21:24].copy())


def project(F, pose12, sR, t, pos, min_dist, max_dist, second_as_depth=False, bounds_scaled=0):
    """cms_sim3s_project over n points -> dict(drop, u, v, dist, raw_max)"""
    pose12 = np.ascontiguousarray(pose12, np.float32).reshape(12); sR = np.ascontiguousarray(sR, np.float32).reshape(9); t = np.ascontiguousarray(t, np.float32).reshape(3)
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); mn = np.ascontiguousarray(min_dist, np.float32); mx = np.ascontiguousarray(max_dist, np.float32)
    n = len(pos)
    u = np.zeros(n, np.float32); v = np.zeros(n, np.float32); d = np.zeros(n, np.float32); raw = np.zeros(n, np.float32); why = np.zeros(n, np.int32)
    H().hm_sim3s_project(F, p(pose12), p(sR), p(t), int(bool(second_as_depth)), int(bounds_scaled), n, p(pos), p(mn), p(mx), p(u), p(v), p(d), p(raw), p(why))
    return dict(drop=why, u=u, v=v, dist=d, raw_max=raw)


def jobs_array(jobs):
    """jobs: dicts with slot1, n1, slot2, n2, s12, R12, t12, off1, off2"""
    arr = (Job * max(len(jobs), 1))()
    for q, j in zip(arr, jobs):
        q.slot1 = j["slot1"]; q.n1 = j["n1"]; q.slot2 = j["slot2"]; q.n2 = j["n2"]; q.s12 = float(j["s12"]); q.off1 = j["off1"]; q.off2 = j["off2"]
        q.R12[:] = [float(x) for x in np.asarray(j["R12"], np.float32).reshape(9)]; q.t12[:] = [float(x) for x in np.asarray(j["t12"], np.float32).reshape(3)]
    return arr


def job_check(jobs, used, slot_n, n_mp, th=7.5, nlevels=8, same_device=True):
    """hm_sim3s_job_check -> (rc, reason)"""
    used = np.ascontiguousarray(used, np.uint8); slot_n = np.ascontiguousarray(slot_n, np.int32)
    buf = C.create_string_buffer(256)
    rc = H().hm_sim3s_job_check(len(jobs), jobs_array(jobs), len(used), p(used), p(slot_n), n_mp, float(th), nlevels, int(same_device), buf, 256)
    return rc, buf.value.decode()
