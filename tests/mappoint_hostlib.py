"""ctypes access to the host build of the map-point core (libcubemapslam_host.so: csrc/cms_mappoint_core.h through host_capi.cpp's hm_mpstore_*
functions), and the two backends of mappoint_cases.run: HostBackend on it, DeviceBackend on a KeyframeStore with an api.Covisibility and an
api.MapPointStore.  A refused call raises Refused on both, with the library's reason where there is one."""
import ctypes as C

import numpy as np

import mappoint_cases as mc
from cubemapslam_amd import api
from hostlib import load, p

_H = None


class Refused(Exception):
    pass


def H():
    global _H
    if _H is None:
        _H = load()
        _H.hm_mpstore_create.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
        _H.hm_mpstore_destroy.argtypes = [C.c_void_p]; _H.hm_mpstore_destroy.restype = None
        _H.hm_mpstore_put.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
        _H.hm_mpstore_update_poses.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _H.hm_mpstore_update_map_points.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
        _H.hm_mpstore_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _H.hm_mpstore_observations.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _H.hm_mpstore_set.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
        _H.hm_mpstore_erase.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _H.hm_mpstore_refresh.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _H.hm_mpstore_fetch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
    return _H


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def _ptr(a):
    return None if a is None or len(a) == 0 else p(a)


def mirror(engine, c, what=mc.BOTH):
    """The mirror's MapPointStore (cubemap_hot_path.h) through one engine on a case: Build over the members, SetMapPoints, Refresh, Fetch -> (status, rows);
    best_member is the index of the row's pBestKF in the member list"""
    from cubemapslam_amd import synth
    assert H().hm_set_camera(C.byref(api.make_camera(synth.camera("lafida", 150)))) == 0, H().hm_last_error()      # the shared context of the device engine wants one
    H().hm_mpstore_mirror.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 7
    M = len(c["rows"])
    n_feat = _i32([len(r) for r in c["rows"]]); mp = _i32(np.concatenate(c["rows"])); oc = _i32(np.concatenate(c["octs"]))
    desc = np.ascontiguousarray(np.concatenate(c["descs"]), np.uint8)
    Tcw = np.tile(np.eye(4, dtype=np.float32), (M, 1, 1))
    for m in range(M):
        Tcw[m, :3, 3] = -c["Ows"][m]      # R = I: Ow = -t, exactly
    Tcw = np.ascontiguousarray(Tcw)
    slot_member = {s: m for m, s in enumerate(c["slots"])}
    ids = _i32(c["ids"]); pos = np.ascontiguousarray(c["pos"], np.float32); ref = _i32([slot_member[int(s)] for s in c["ref"]])
    n = len(ids)
    o = mc.empty_rows(n)
    status = np.zeros(n, np.uint8)
    rc = H().hm_mpstore_mirror(int(engine), M, p(n_feat), p(mp), p(oc), p(desc), p(Tcw), mc.MAX_POINTS, n, p(ids), p(pos), p(ref), int(what), p(status), p(o["normal"]),
                               p(o["min_dist"]), p(o["max_dist"]), p(o["desc"]), p(o["best_member"]), p(o["best_feature"]))
    assert rc == 0, H().hm_last_error().decode()
    o["pos"] = pos.copy()
    return status, o


class HostBackend:
    """CmsMpHostStore behind the calls of the C-ABI"""

    def __init__(self, K=mc.K, max_features=mc.MAXF, max_points=mc.MAX_POINTS):
        self.h = C.c_void_p()
        sf = np.ascontiguousarray(mc.SF, np.float32)
        assert H().hm_mpstore_create(C.byref(self.h), K, max_features, K, max_points, mc.NLEVELS, p(sf)) == 0

    def close(self):
        if self.h:
            H().hm_mpstore_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise Refused("code %d" % rc)

    def put(self, slot, mp, octave, desc, Ow):
        a = [_i32(mp), _i32(octave), np.ascontiguousarray(desc, np.uint8), np.ascontiguousarray(Ow, np.float32)]
        self._chk(H().hm_mpstore_put(self.h, int(slot), len(a[0]), _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), p(a[3])))

    def update_poses(self, slots, Ows):
        s = _i32(slots); o = np.ascontiguousarray(Ows, np.float32).reshape(-1)
        self._chk(H().hm_mpstore_update_poses(self.h, len(s), p(s), p(o)))

    def update_map_points(self, slot, feat, mp):
        a = [_i32(slot), _i32(feat), _i32(mp)]
        self._chk(H().hm_mpstore_update_map_points(self.h, len(a[0]), p(a[0]), p(a[1]), p(a[2])))

    def build(self, slots):
        s = _i32(slots)
        self._chk(H().hm_mpstore_build(self.h, len(s), _ptr(s)))

    def load(self, c):
        for s, r, o, d, w in zip(c["slots"], c["rows"], c["octs"], c["descs"], c["Ows"]):
            self.put(s, r, o, d, w)
        self.build(c["slots"])

    def observations(self, id_, cap=16384):
        out = np.zeros(3 * cap, np.int32); n = C.c_int()
        self._chk(H().hm_mpstore_observations(self.h, int(id_), cap, p(out), C.byref(n)))
        return [tuple(int(v) for v in out[3 * k:3 * k + 3]) for k in range(n.value)]

    def set(self, ids, pos=None, ref=None):
        ids = _i32(ids)
        pos = None if pos is None else np.ascontiguousarray(pos, np.float32).reshape(-1)
        ref = None if ref is None else _i32(ref)
        self._chk(H().hm_mpstore_set(self.h, len(ids), _ptr(ids), _ptr(pos), _ptr(ref)))

    def erase(self, ids):
        ids = _i32(ids)
        self._chk(H().hm_mpstore_erase(self.h, len(ids), _ptr(ids)))

    def refresh(self, ids, what=mc.BOTH):
        ids = _i32(ids)
        status = np.zeros(max(len(ids), 1), np.uint8)
        self._chk(H().hm_mpstore_refresh(self.h, len(ids), _ptr(ids), int(what), p(status)))
        return status[:len(ids)]

    def fetch(self, ids):
        ids = _i32(ids)
        o = mc.empty_rows(len(ids))
        self._chk(H().hm_mpstore_fetch(self.h, len(ids), _ptr(ids), *[p(o[k]) for k in ("pos", "normal", "min_dist", "max_dist", "desc", "best_member", "best_feature")]))
        return o


def keyframe(mp, octave, desc, Ow, x=None, y=None, R=None, t=None):
    """what fills a slot: the mp row, octaves, descriptors and camera centre the refresh reads; key points inside the image, no FeatureVector"""
    n = len(mp)
    i = np.arange(n)
    Ow = np.asarray(Ow, np.float32)
    kf = dict(x=(10 + i % 400).astype(np.float32) if x is None else x, y=(10 + i // 400).astype(np.float32) if y is None else y, octave=np.asarray(octave, np.int32),
              angle=np.zeros(n, np.float32), desc=np.ascontiguousarray(desc, np.uint8).reshape(n, 32), rays=np.tile(np.array([0, 0, 1], np.float32), (n, 1)),
              mp=np.asarray(mp, np.int32), R=np.eye(3, dtype=np.float32) if R is None else R, t=(-Ow) if t is None else t, Ow=Ow, median_depth=1.0,
              node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32))
    return api.make_keyframe(kf)


class DeviceBackend:
    """mappoint_cases.run on a KeyframeStore; load() starts a fresh index and a fresh table"""

    def __init__(self, store, max_members, max_points=mc.MAX_POINTS):
        self.st, self.max_members, self.max_points = store, max_members, max_points
        self.cv = self.mp = None
        self.reset()

    def reset(self):
        self.close()
        self.cv = api.Covisibility(self.st, self.max_members)
        self.mp = api.MapPointStore(self.st, self.max_points)

    def close(self):
        if self.mp is not None:
            self.mp.close(); self.cv.close()
            self.cv = self.mp = None

    def _call(self, f, *a):
        try:
            return f(*a)
        except api.CmsError as e:
            raise Refused(str(e))

    def put(self, slot, mp, octave, desc, Ow):
        K, keep = keyframe(mp, octave, desc, Ow)
        self._call(self.st.put, int(slot), K)

    def update_poses(self, slots, Ows):
        Ows = np.ascontiguousarray(Ows, np.float32).reshape(-1, 3)
        self._call(self.st.update_poses, slots, np.tile(np.eye(3, dtype=np.float32).reshape(9), (len(Ows), 1)), -Ows, Ows)

    def update_map_points(self, slot, feat, mp): self._call(self.st.update_map_points, slot, feat, mp)
    def build(self, slots): self._call(self.cv.build, slots)

    def load(self, c):
        self.reset()
        for s, r, o, d, w in zip(c["slots"], c["rows"], c["octs"], c["descs"], c["Ows"]):
            self.put(s, r, o, d, w)
        self.build(c["slots"])

    def set(self, ids, pos=None, ref=None): self._call(self.mp.set, ids, pos, ref)
    def erase(self, ids): self._call(self.mp.erase, ids)
    def refresh(self, ids, what=mc.BOTH): return self._call(self.mp.refresh, self.cv, ids, what)
    def fetch(self, ids): return self._call(self.mp.fetch, ids)
