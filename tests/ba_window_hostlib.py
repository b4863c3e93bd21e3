"""ctypes access to the host build of the local-BA-window core (libcubemapslam_host.so: csrc/cms_ba_window_core.h through host_capi.cpp's
hm_ba_window_* functions) and the device side of a case of tests/ba_window_cases.py: a KeyframeStore filled with the case's members, an
api.Covisibility built over them and an api.MapPointStore holding the positions."""
import ctypes as C

import numpy as np

import ba_window_cases as bc
from cubemapslam_amd import api
from hostlib import load, p

_H = None


class Refused(Exception):
    pass


def H():
    global _H
    if _H is None:
        _H = load()
        _H.hm_ba_window_create.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _H.hm_ba_window_destroy.argtypes = [C.c_void_p]; _H.hm_ba_window_destroy.restype = None
        _H.hm_ba_window_run.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 12
        _H.hm_init_cos_fov.restype = C.c_float; _H.hm_init_cos_fov.argtypes = [C.c_double]
    return _H


def set_camera(camd=None):
    """the host library's one camera (face width, cos_fov): other test modules set theirs, so every entry point here sets its own first"""
    assert H().hm_set_camera(C.byref(api.make_camera(bc.CAMD if camd is None else camd))) == 0, H().hm_last_error()


def cos_fov():
    return float(H().hm_init_cos_fov(float(bc.CAMD["fov_deg"])))


def _ptr(a):
    return None if a is None or len(a) == 0 else p(a)


def trim(o, nj):
    """the windows of filled output arrays (api.ba_window_arrays), cut to their counts and copied"""
    res = []
    for j in range(nj):
        K, _, P, E = (int(v) for v in o["counts"][j])
        w = dict(counts=o["counts"][j].copy())
        for k, n in (("kf_member", K), ("poses", K), ("fixed", K), ("point_id", P), ("points", P), ("e_pose", E), ("e_point", E), ("e_obs", E), ("e_invsig2", E), ("e_face", E),
                     ("e_feat", E)):
            w[k] = o[k][j, :min(n, o[k].shape[1])].copy()
        res.append(w)
    return res


class HostWindows:
    """the host core over a case; run(jobs, caps) -> (code, windows, raw output arrays)"""

    def __init__(self, c, inv_sigma2=bc.INV_SIGMA2, pos_ids=None, pos=None):
        set_camera()
        a = bc.concat(c)
        ids = np.ascontiguousarray(c["pos_ids"] if pos_ids is None else pos_ids, np.int32)
        pos = np.ascontiguousarray(c["pos"] if pos is None else pos, np.float32).reshape(-1)
        inv = np.ascontiguousarray(inv_sigma2, np.float32)
        self.h = C.c_void_p()
        rc = H().hm_ba_window_create(C.byref(self.h), len(a["n"]), p(a["n"]), _ptr(a["mp"]), _ptr(a["oct"]), _ptr(a["x"]), _ptr(a["y"]), _ptr(a["ray_z"]), p(a["R"]), p(a["t"]),
                                     c["max_points"], len(ids), _ptr(ids), _ptr(pos), bc.NLEVELS, p(inv))
        assert rc == 0, H().hm_last_error().decode()

    def close(self):
        if self.h:
            H().hm_ba_window_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, jobs, caps, out=None):
        nj = len(jobs)
        off = np.concatenate([[0], np.cumsum([len(j[0]) for j in jobs])]).astype(np.int32)
        mem = np.ascontiguousarray(np.concatenate([np.asarray(j[0], np.int32) for j in jobs] + [np.zeros(0, np.int32)]), np.int32)
        first = np.array([j[1] for j in jobs] + [0], np.int32)
        o = api.ba_window_arrays(nj, *caps) if out is None else out
        rc = H().hm_ba_window_run(self.h, nj, p(off), _ptr(mem), p(first), int(caps[0]), int(caps[1]), int(caps[2]), *[p(o[k]) for k in ("counts",) + api.BA_WINDOW_ARRAYS])
        if rc == -1:
            raise Refused(H().hm_last_error().decode())
        assert rc in (0, -4), rc
        return rc, trim(o, nj), o


def host_windows(c, jobs=None, caps=None):
    hw = HostWindows(c)
    rc, w, _ = hw.run(c["jobs"] if jobs is None else jobs, c["caps"] if caps is None else caps)
    hw.close()
    return rc, w


def keyframe(m):
    """a case's member as what fills a slot; descriptors are zero, the FeatureVector is empty"""
    n = len(m["mp"])
    R = np.asarray(m["R"], np.float32); t = np.asarray(m["t"], np.float32)
    kf = dict(x=m["x"], y=m["y"], octave=m["oct"], angle=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), rays=m["rays"], mp=m["mp"], R=R, t=t,
              Ow=(-R.T @ t).astype(np.float32), median_depth=1.0, node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32))
    return api.make_keyframe(kf)


class DeviceMap:
    """a case on the device: store, index, table"""

    def __init__(self, ctx, c, max_members=None):
        self.c = c
        self.st = api.KeyframeStore(ctx, max_keyframes=c["K"], max_features=c["maxf"], max_nodes=8)
        for s, m in zip(c["slots"], c["members"]):
            K, keep = keyframe(m)
            self.st.put(s, K)
            del keep
        self.cv = api.Covisibility(self.st, max_members or len(c["members"]))
        self.cv.build(c["slots"])
        self.mp = api.MapPointStore(self.st, c["max_points"])
        if len(c["pos_ids"]):
            self.mp.set(c["pos_ids"], c["pos"], c["ref"])

    def windows(self, jobs=None, caps=None, pinned=False, out=None):
        return self.cv.local_ba_windows(self.mp, self.c["jobs"] if jobs is None else jobs, *(self.c["caps"] if caps is None else caps), pinned=pinned, out=out)

    def close(self):
        self.mp.close(); self.cv.close(); self.st.close()


def mirror(engine, c, local, mn_ids=None, run_ba=False, caps=None, camd=None):
    """MapPointStore::LocalBAWindow of the mirror (host/cubemap_hot_path.h) through one engine (0 device, 1 host core) on a case's members and points
    -> the window; key frame `first` of mn_ids == 0 is the map's first.  run_ba: Optimizer::LocalBundleAdjustment behind it -> (window, n_erase, Tcw)"""
    H().hm_ba_window_mirror.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int] + [C.c_int] * 3 + \
        [C.c_void_p] * 14
    set_camera(camd)
    ms = c["members"]
    M = len(ms)
    a = bc.concat(c)
    rays = np.ascontiguousarray(np.concatenate([np.asarray(m["rays"], np.float32).reshape(-1, 3) for m in ms]), np.float32)
    Tcw = np.tile(np.eye(4, dtype=np.float32), (M, 1, 1))
    for k, m in enumerate(ms):
        Tcw[k, :3, :3] = m["R"]; Tcw[k, :3, 3] = m["t"]
    Tcw = np.ascontiguousarray(Tcw)
    mn = np.ascontiguousarray(np.arange(1, M + 1) if mn_ids is None else mn_ids, np.int32)
    ids = np.ascontiguousarray(c["pos_ids"], np.int32); pos = np.ascontiguousarray(c["pos"], np.float32)
    ref = np.ascontiguousarray([c["slots"].index(int(s)) for s in c["ref"]], np.int32)
    loc = np.ascontiguousarray(local, np.int32)
    caps = caps or (M, int(sum(len(ms[k]["mp"]) for k in local)) + 1, 16 * int(sum(len(ms[k]["mp"]) for k in local)) + 16)
    o = api.ba_window_arrays(1, *caps)
    n_erase = C.c_int()
    Tout = np.zeros_like(Tcw)
    rc = H().hm_ba_window_mirror(int(engine), M, p(a["n"]), _ptr(a["mp"]), _ptr(a["oct"]), _ptr(a["x"]), _ptr(a["y"]), _ptr(rays), p(Tcw), p(mn), c["max_points"], len(ids),
                                 _ptr(ids), _ptr(pos), _ptr(ref), len(loc), p(loc), 1 if run_ba else 0, *caps, *[p(o[k]) for k in ("counts",) + api.BA_WINDOW_ARRAYS],
                                 C.byref(n_erase), p(Tout))
    assert rc == 0, (rc, H().hm_last_error().decode())
    w = trim(o, 1)[0]
    return (w, n_erase.value, Tout) if run_ba else w
