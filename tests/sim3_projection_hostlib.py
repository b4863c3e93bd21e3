"""ctypes access to the host build of the SearchByProjection(Scw) / Fuse(Scw) core and job check (libcubemapslam_host.so:
cubemapslam_amd/host/sim3_proj_host.cpp)."""
import ctypes as C

import numpy as np

from hostlib import load, p
from npref_reloc import logf

_H = None


class Job(C.Structure):
    """cms_sim3_proj_job (include/cubemapslam_hip.h)"""
    _fields_ = [("slot", C.c_int), ("n", C.c_int), ("Scw", C.c_float * 12), ("set", C.c_int)]


def H():
    global _H
    if _H is None:
        _H = load()
        _H.hm_sim3p_decompose.argtypes = [C.c_void_p, C.c_void_p]
        _H.hm_sim3p_decompose.restype = None
        _H.hm_sim3p_project.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 10
        _H.hm_sim3p_project.restype = None
        _H.hm_sim3p_job_check.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_char_p, C.c_int]
        assert _H.hm_sim3p_pose_size() == 16 * 4 and _H.hm_sim3p_job_size() == C.sizeof(Job)
    return _H


def decompose(Scw):
    """cms_sim3p_decompose -> dict(scw, Rcw, tcw, Ow)"""
    S = np.ascontiguousarray(np.asarray(Scw, np.float32).reshape(-1)[:12])
    out = np.zeros(16, np.float32)
    H().hm_sim3p_decompose(p(S), p(out))
    return dict(Rcw=out[:9].reshape(3, 3).copy(), tcw=out[9:12].copy(), Ow=out[12:15].copy(), scw=out[15])


def project(F, Scw, pos, normal, min_dist, max_dist, th, sf, bounds_scaled=0):
    """cms_sim3p_project over n points -> dict(drop, u, v, dist, level, radius)"""
    S = np.ascontiguousarray(np.asarray(Scw, np.float32).reshape(-1)[:12]); sf = np.ascontiguousarray(sf, np.float32)
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); nrm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    mn = np.ascontiguousarray(min_dist, np.float32); mx = np.ascontiguousarray(max_dist, np.float32)
    n = len(pos)
    u = np.zeros(n, np.float32); v = np.zeros(n, np.float32); d = np.zeros(n, np.float32); r = np.zeros(n, np.float32)
    lvl = np.zeros(n, np.int32); why = np.zeros(n, np.int32)
    H().hm_sim3p_project(F, p(S), int(bounds_scaled), float(th), float(logf(sf[1])), len(sf), p(sf), n, p(pos), p(nrm), p(mn), p(mx), p(u), p(v), p(d), p(lvl), p(r), p(why))
    return dict(drop=why, u=u, v=v, dist=d, level=lvl, radius=r)


def jobs_array(jobs):
    """jobs: dicts with slot, n, Scw, set"""
    arr = (Job * max(len(jobs), 1))()
    for q, j in zip(arr, jobs):
        q.slot = j["slot"]; q.n = j["n"]; q.set = j["set"]
        q.Scw[:] = [float(x) for x in np.asarray(j["Scw"], np.float32).reshape(-1)[:12]]
    return arr


def job_check(jobs, used, slot_n, set_off, th=10.0, nlevels=8, same_device=True):
    """hm_sim3p_job_check -> (rc, reason)"""
    used = np.ascontiguousarray(used, np.uint8); slot_n = np.ascontiguousarray(slot_n, np.int32); set_off = np.ascontiguousarray(set_off, np.int32)
    buf = C.create_string_buffer(256)
    rc = H().hm_sim3p_job_check(len(jobs), jobs_array(jobs), len(used), p(used), p(slot_n), len(set_off) - 1, p(set_off), float(th), nlevels, int(same_device), buf, 256)
    return rc, buf.value.decode()
