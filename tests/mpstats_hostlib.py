"""ctypes access to the host build of the map-point statistics (libcubemapslam_host.so: csrc/cms_mpstats_core.h through host_capi.cpp's hm_mpstats_*
functions on the handle of hm_mpstore_*), and the two real backends of mpstats_cases' runner: HostBackend on it, DeviceBackend on a KeyframeStore
with an api.Covisibility and an api.MapPointStore.  The third backend is the restatement, npref_mpstats.Model.  A refused call raises Refused on
both, with the library's reason on the device."""
import ctypes as C

import numpy as np

import mpstats_cases as sc
from cubemapslam_amd import api
from hostlib import load, p
from mappoint_hostlib import Refused, keyframe

_H = None
f32 = np.float32


def H():
    global _H
    if _H is None:
        import mappoint_hostlib
        _H = mappoint_hostlib.H()      # (declares hm_mpstore_*)
        V, I = C.c_void_p, C.c_int
        _H.hm_mpstats_update_poses.argtypes = [V, I, V, V, V, V]
        _H.hm_mpstats_set_stats.argtypes = [V, I, V, V, V, V]
        _H.hm_mpstats_add_stats.argtypes = [V, I, V, V, V]
        _H.hm_mpstats_fetch_stats.argtypes = [V, I, V, V, V, V]
        _H.hm_mpstats_count.argtypes = [V, I, I, V, V, V, I]
        _H.hm_mpstats_culling.argtypes = [V, I, V, V, V, I, I, V]
        _H.hm_mpstats_tracked_map_points.argtypes = [V, I, V, V, V]
        _H.hm_mpstats_scene_median_depth.argtypes = [V, I, V, I, I, V, V]
        _H.hm_mpstats_fetch_mp.argtypes = [V, I, I, V, V]
        _H.hm_mpstats_fetch_median.argtypes = [V, I, V]
    return _H


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def _opt(a):
    return None if a is None else _i32(a)


def _ptr(a):
    return None if a is None or len(a) == 0 else p(a)


def camera_centre(R, t):
    return (-(np.asarray(R, np.float64).reshape(3, 3).T @ np.asarray(t, np.float64))).astype(f32)


def _pose(R, t):
    R = np.eye(3, dtype=f32) if R is None else np.ascontiguousarray(R, f32).reshape(3, 3)
    t = np.zeros(3, f32) if t is None else np.ascontiguousarray(t, f32).reshape(3)
    return R, t, camera_centre(R, t)


def _csr(lists, flags):
    off, ids = api._csr(lists)
    fl = None
    if flags is not None:
        fl = np.zeros(len(ids), np.uint8)
        if int(off[-1]):
            fl[:-1] = np.concatenate([np.asarray(f, np.uint8).reshape(-1) for f in flags if len(f)])
    return off, ids, fl


class HostBackend:
    """CmsMpHostStore behind the calls of the C-ABI"""

    def __init__(self, K, maxf, max_points):
        self.h = C.c_void_p()
        sf = np.ascontiguousarray(sc.SF, f32)
        assert H().hm_mpstore_create(C.byref(self.h), K, maxf, K, max_points, sc.NLEVELS, p(sf)) == 0

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

    def put(self, slot, mp, octave=None, R=None, t=None):
        mp = _i32(mp)
        oc = np.zeros(len(mp), np.int32) if octave is None else _i32(octave)
        R, t, Ow = _pose(R, t)
        desc = np.zeros((max(len(mp), 1), 32), np.uint8)
        self._chk(H().hm_mpstore_put(self.h, int(slot), len(mp), _ptr(mp), _ptr(oc), p(desc), p(Ow)))
        self.update_poses([slot], R, t)

    def update_poses(self, slots, R, t):
        s = _i32(slots)
        R = np.ascontiguousarray(R, f32).reshape(-1, 3, 3); t = np.ascontiguousarray(t, f32).reshape(-1, 3)
        Ow = np.ascontiguousarray(np.stack([camera_centre(r, tt) for r, tt in zip(R, t)]), f32)
        self._chk(H().hm_mpstats_update_poses(self.h, len(s), p(s), p(R), p(t), p(Ow)))

    def update_map_points(self, slot, feat, mp):
        a = [_i32(slot), _i32(feat), _i32(mp)]
        self._chk(H().hm_mpstore_update_map_points(self.h, len(a[0]), p(a[0]), p(a[1]), p(a[2])))

    def fetch_mp(self, slot):
        out = np.zeros(16384, np.int32); n = C.c_int()
        self._chk(H().hm_mpstats_fetch_mp(self.h, int(slot), len(out), p(out), C.byref(n)))
        return out[:n.value].copy()

    def build(self, slots):
        s = _i32(slots)
        self._chk(H().hm_mpstore_build(self.h, len(s), _ptr(s)))

    def observations(self, id_):
        out = np.zeros(3, np.int32); n = C.c_int()
        self._chk(H().hm_mpstore_observations(self.h, int(id_), 1, p(out), C.byref(n)))
        return n.value

    def set(self, ids, pos=None, ref=None):
        ids = _i32(ids)
        pos = None if pos is None else np.ascontiguousarray(pos, f32).reshape(-1)
        self._chk(H().hm_mpstore_set(self.h, len(ids), _ptr(ids), _ptr(pos), _ptr(_opt(ref))))

    def erase(self, ids):
        ids = _i32(ids)
        self._chk(H().hm_mpstore_erase(self.h, len(ids), _ptr(ids)))

    def set_stats(self, ids, first_kf=None, visible=None, found=None):
        ids = _i32(ids)
        self._chk(H().hm_mpstats_set_stats(self.h, len(ids), _ptr(ids), _ptr(_opt(first_kf)), _ptr(_opt(visible)), _ptr(_opt(found))))

    def add_stats(self, ids, d_visible=None, d_found=None):
        ids = _i32(ids)
        self._chk(H().hm_mpstats_add_stats(self.h, len(ids), _ptr(ids), _ptr(_opt(d_visible)), _ptr(_opt(d_found))))

    def fetch_stats(self, ids):
        ids = _i32(ids)
        o = [np.zeros(max(len(ids), 1), np.int32) for _ in range(3)]
        self._chk(H().hm_mpstats_fetch_stats(self.h, len(ids), _ptr(ids), p(o[0]), p(o[1]), p(o[2])))
        return tuple(v[:len(ids)] for v in o)

    def count(self, which, id_lists, flags=None, count_if=1, ctx=0):
        off, ids, fl = _csr(id_lists, flags)
        self._chk(H().hm_mpstats_count(self.h, int(which), len(id_lists), p(off), p(ids), None if fl is None else p(fl), int(count_if)))

    def culling(self, id_lists, current_kf, th_obs=2, apply=False):
        off, ids, _ = _csr(id_lists, None)
        cur = np.zeros(len(id_lists) + 1, np.int32); cur[:-1] = current_kf
        v = np.zeros(len(ids), np.uint8)
        self._chk(H().hm_mpstats_culling(self.h, len(id_lists), p(off), p(ids), p(cur), int(th_obs), int(bool(apply)), p(v)))
        return [v[off[j]:off[j + 1]].copy() for j in range(len(id_lists))]

    def tracked(self, members, min_obs, ctx=0):
        m = _i32(members)
        mo = np.ascontiguousarray(np.broadcast_to(np.asarray(min_obs, np.int32), m.shape))
        out = np.zeros(max(len(m), 1), np.int32)
        self._chk(H().hm_mpstats_tracked_map_points(self.h, len(m), _ptr(m), _ptr(mo), p(out)))
        return out[:len(m)]

    def median_depth(self, slots, q=2, store=False):
        s = _i32(slots)
        d = np.zeros(max(len(s), 1), f32); n = np.zeros(max(len(s), 1), np.int32)
        self._chk(H().hm_mpstats_scene_median_depth(self.h, len(s), _ptr(s), int(q), int(bool(store)), p(d), p(n)))
        return d[:len(s)], n[:len(s)]

    def stored_median(self, slot):
        v = C.c_float()
        self._chk(H().hm_mpstats_fetch_median(self.h, int(slot), C.byref(v)))
        return f32(v.value)


class DeviceBackend:
    """the runner on a KeyframeStore; reset() starts a fresh index and a fresh table.  ctxs: the frame contexts whose streams count, tracked and
    observations run on"""

    def __init__(self, store, ctxs, max_members, max_points):
        self.st, self.ctxs, self.max_members, self.max_points = store, ctxs, max_members, max_points
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

    def _call(self, f, *a, **kw):
        try:
            return f(*a, **kw)
        except api.CmsError as e:
            raise Refused(str(e))

    def put(self, slot, mp, octave=None, R=None, t=None):
        mp = _i32(mp)
        oc = np.zeros(len(mp), np.int32) if octave is None else _i32(octave)
        R, t, Ow = _pose(R, t)
        K, keep = keyframe(mp, oc, np.zeros((len(mp), 32), np.uint8), Ow, R=R, t=t)
        self._call(self.st.put, int(slot), K)

    def update_poses(self, slots, R, t):
        R = np.ascontiguousarray(R, f32).reshape(-1, 3, 3); t = np.ascontiguousarray(t, f32).reshape(-1, 3)
        self._call(self.st.update_poses, slots, R, t, np.stack([camera_centre(r, tt) for r, tt in zip(R, t)]))

    def update_map_points(self, slot, feat, mp): self._call(self.st.update_map_points, slot, feat, mp)
    def fetch_mp(self, slot): return self.st.debug_fetch(int(slot))["mp"]
    def build(self, slots): self._call(self.cv.build, slots)
    def observations(self, id_): return int(self._call(self.cv.votes, self.ctxs[0], [[int(id_)]]).sum())
    def set(self, ids, pos=None, ref=None): self._call(self.mp.set, ids, pos, ref)
    def erase(self, ids): self._call(self.mp.erase, ids)
    def set_stats(self, ids, first_kf=None, visible=None, found=None): self._call(self.mp.set_stats, ids, first_kf, visible, found)
    def add_stats(self, ids, d_visible=None, d_found=None): self._call(self.mp.add_stats, ids, d_visible, d_found)
    def fetch_stats(self, ids): return self._call(self.mp.fetch_stats, ids)
    def count(self, which, id_lists, flags=None, count_if=1, ctx=0): self._call(self.mp.count, self.ctxs[ctx], which, id_lists, flags, count_if)
    def culling(self, id_lists, current_kf, th_obs=2, apply=False): return self._call(self.mp.culling, self.cv, id_lists, current_kf, th_obs, apply)
    def tracked(self, members, min_obs, ctx=0): return self._call(self.cv.tracked_map_points, self.ctxs[ctx], members, min_obs)
    def median_depth(self, slots, q=2, store=False): return self._call(self.st.scene_median_depth, self.mp, slots, q, store)


def mirror_case():
    """one mapping step for the mirror: four key frames of 40 to 120 features over 90 points, first key frames 0..3, six frames of ids with flags"""
    rng = np.random.default_rng(17)
    n_pts = 90
    n_feat = [120, 80, 64, 40]
    rows = []
    for n in n_feat:
        r = np.full(n, -1, np.int32)
        k = int(0.7 * n)
        r[rng.choice(n, k, replace=False)] = rng.choice(n_pts, k, replace=False)
        rows.append(r)
    Tcw = np.tile(np.eye(4, dtype=f32), (4, 1, 1))
    for k in range(4):
        Tcw[k, :3, :3] = sc.rotation(100 + k); Tcw[k, :3, 3] = rng.normal(0, 1, 3)
    frames = [np.where(rng.random(150) < 0.85, rng.integers(0, n_pts, 150), -1).astype(np.int32) for _ in range(6)]
    return dict(n_feat=_i32(n_feat), mp=_i32(np.concatenate(rows)), octave=_i32(rng.integers(0, sc.NLEVELS, sum(n_feat))), Tcw=np.ascontiguousarray(Tcw),
                ids=_i32(np.arange(n_pts)), pos=np.ascontiguousarray(rng.normal(0, 3, (n_pts, 3)), f32), first_kf=_i32(rng.integers(0, 4, n_pts)),
                frame_off=_i32(np.concatenate([[0], np.cumsum([len(x) for x in frames])])), frame_ids=_i32(np.concatenate(frames)),
                in_view=(rng.random(900) < 0.7).astype(np.uint8), outlier=(rng.random(900) < 0.7).astype(np.uint8), current_kf=4, min_obs=2, q=2, rows=rows)


def mirror(engine, c):
    """CubemapSLAM::MapPointStore's statistics methods (cubemap_hot_path.h) through one engine -> [(label, value)] for mpstats_cases.difference"""
    from cubemapslam_amd import synth
    assert H().hm_set_camera(C.byref(api.make_camera(synth.camera("lafida", 150)))) == 0, H().hm_last_error()      # the shared context of the device engine wants one
    V, I = C.c_void_p, C.c_int
    H().hm_mpstats_mirror.argtypes = [I, I, V, V, V, V, I, I, V, V, V, I, V, V, V, V, I, I, I, V, V, V, V, V, V]
    n = len(c["ids"])
    verdict = np.zeros(n, np.uint8); stats = np.zeros((n, 3), np.int32); n_left = C.c_int(); mp_out = np.zeros(len(c["mp"]), np.int32)
    tracked = np.zeros(4, np.int32); depth = np.zeros(4, f32)
    rc = H().hm_mpstats_mirror(int(engine), 4, p(c["n_feat"]), p(c["mp"]), p(c["octave"]), p(c["Tcw"]), 1024, n, p(c["ids"]), p(c["pos"]), p(c["first_kf"]),
                               len(c["frame_off"]) - 1, p(c["frame_off"]), p(c["frame_ids"]), p(c["in_view"]), p(c["outlier"]), c["current_kf"], c["min_obs"], c["q"],
                               p(verdict), p(stats), C.byref(n_left), p(mp_out), p(tracked), p(depth))
    assert rc == 0, H().hm_last_error().decode()
    return [("verdict", verdict), ("stats", stats), ("n_left", np.array([n_left.value])), ("mp", mp_out), ("tracked", tracked), ("depth", depth)]


def mirror_expected(c):
    """the same step on the restatement"""
    import npref_mpstats as ref
    m = ref.Model(5, 128, 1024)
    for k, row in enumerate(c["rows"]):
        m.put(k, row, None, c["Tcw"][k, :3, :3], c["Tcw"][k, :3, 3])
    m.build(range(4))
    m.set(c["ids"], c["pos"])
    m.set_stats(c["ids"], first_kf=c["first_kf"])
    off = c["frame_off"]
    for f in range(len(off) - 1):
        s = slice(off[f], off[f + 1])
        m.count(sc.VISIBLE, [c["frame_ids"][s]], [c["in_view"][s]], 1)
        m.count(sc.FOUND, [c["frame_ids"][s]], [c["outlier"][s]], 0)
    v = m.culling([c["ids"]], [c["current_kf"]], 2, True)[0]
    stats = np.stack(m.fetch_stats(c["ids"]), axis=1)[:, [2, 0, 1]]
    mp = np.concatenate([m.fetch_mp(k) for k in range(4)])
    m.build(range(4))
    return [("verdict", v), ("stats", stats), ("n_left", np.array([int((v == 0).sum())])), ("mp", mp), ("tracked", m.tracked(range(4), c["min_obs"])),
            ("depth", m.median_depth(range(4), c["q"])[0])]
