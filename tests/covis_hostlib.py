"""ctypes access to the host build of the covisibility core (libcubemapslam_host.so: csrc/cms_covis_core.h through host_capi.cpp's hm_covis_*
functions), and the two backends of covis_cases.run: HostBackend on it, DeviceBackend on a KeyframeStore with an api.Covisibility."""
import ctypes as C

import numpy as np

import covis_cases as cc
from cubemapslam_amd import api, synth
from hostlib import load, p

_H = None


def H():
    global _H
    if _H is None:
        _H = load()
        _H.hm_covis_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        _H.hm_covis_destroy.argtypes = [C.c_void_p]; _H.hm_covis_destroy.restype = None
        _H.hm_covis_put.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _H.hm_covis_update_map_points.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
        _H.hm_covis_fetch_mp.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _H.hm_covis_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _H.hm_covis_votes.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
        _H.hm_covis_connections.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        _H.hm_covis_culling.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3
        _H.hm_covis_local_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _H.hm_covis_mirror.argtypes = ([C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int] +
                                       [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
    return _H


def mirror(engine, rows, octs, conn_kf, cull_kf, not_erase, frame_ids, lp_kf):
    """The mirror's Covisibility (cubemap_hot_path.h) through one engine: (ordered connections of conn_kf concatenated, their weights, their counts,
    nMPs, nRedundantObservations, verdicts, local key frames, pKFmax, local points)"""
    i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)
    assert H().hm_set_camera(C.byref(api.make_camera(synth.camera("lafida", 150)))) == 0, H().hm_last_error()      # the shared context of the device engine wants one
    n_feat = i32([len(r) for r in rows]); mp = i32(np.concatenate(rows)); oc = i32(np.concatenate(octs))
    M = len(rows)
    conn = i32(conn_kf); cull = i32(cull_kf); ne = np.ascontiguousarray(not_erase, np.uint8); ids = i32(frame_ids); lp = i32(lp_kf)
    ordered = np.zeros(len(conn) * M + 1, np.int32); ordered_w = np.zeros(len(conn) * M + 1, np.int32); n_ord = np.zeros(len(conn) + 1, np.int32)
    nm = np.zeros(len(cull) + 1, np.int32); nr = np.zeros(len(cull) + 1, np.int32); red = np.zeros(len(cull) + 1, np.uint8)
    local = np.zeros(M + 1, np.int32); n_local, kf_max, n_lp = C.c_int(), C.c_int(), C.c_int()
    cap = int(n_feat.sum()) + 1
    lp_ids = np.zeros(cap, np.int32)
    rc = H().hm_covis_mirror(int(engine), M, p(n_feat), p(mp), p(oc), len(conn), p(conn), p(ordered), p(ordered_w), p(n_ord), len(cull), p(cull), p(ne), p(nm), p(nr), p(red),
                             len(ids), p(ids), p(local), C.byref(n_local), C.byref(kf_max), len(lp), p(lp), cap, p(lp_ids), C.byref(n_lp))
    assert rc == 0, H().hm_last_error().decode()
    t = int(n_ord[:len(conn)].sum())
    return ([int(v) for v in ordered[:t]], [int(v) for v in ordered_w[:t]], [int(v) for v in n_ord[:len(conn)]], nm[:len(cull)], nr[:len(cull)], red[:len(cull)],
            [int(v) for v in local[:n_local.value]], kf_max.value, [int(v) for v in lp_ids[:n_lp.value]])


class HostBackend:
    """CmsCovisHostStore behind the calls of the C-ABI; put / update_map_points / build return the call's code"""

    def __init__(self, K=cc.K, max_features=cc.MAXF, max_members=None):
        self.h = C.c_void_p()
        assert H().hm_covis_create(C.byref(self.h), K, max_features, K if max_members is None else max_members) == 0
        self.M = 0

    def close(self):
        if self.h:
            H().hm_covis_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def put(self, slot, mp, octave):
        mp = np.ascontiguousarray(mp, np.int32); octave = np.ascontiguousarray(octave, np.int32)
        pad = lambda a: p(a) if len(a) else None
        return H().hm_covis_put(self.h, int(slot), len(mp), pad(mp), pad(octave))

    def update_map_points(self, slot, feat, mp):
        a = [np.ascontiguousarray(v, np.int32).reshape(-1) for v in (slot, feat, mp)]
        return H().hm_covis_update_map_points(self.h, len(a[0]), p(a[0]), p(a[1]), p(a[2]))

    def fetch_mp(self, slot, n):
        out = np.zeros(n, np.int32)
        assert H().hm_covis_fetch_mp(self.h, int(slot), p(out)) == 0
        return out

    def build(self, slots):
        s = np.ascontiguousarray(slots, np.int32).reshape(-1)
        rc = H().hm_covis_build(self.h, len(s), p(s) if len(s) else None)
        if rc == 0:
            self.M = len(s)
        return rc

    def load(self, c):
        for s, r, o in zip(c["slots"], c["rows"], c["octs"]):
            assert self.put(s, r, o) == 0
        return self.build(c["slots"])

    def votes(self, id_lists, code=False):
        off, ids = cc.offsets(id_lists)
        out = np.zeros((len(id_lists), self.M), np.int32)
        rc = H().hm_covis_votes(self.h, len(id_lists), p(off), p(ids), p(out) if out.size else None)
        if code:
            return rc
        assert rc == 0
        return out

    def connections(self, members, th):
        m = np.ascontiguousarray(members, np.int32)
        w = np.zeros((len(m), self.M), np.int32); order = np.full((len(m), self.M), -1, np.int32); nc = np.zeros(len(m), np.int32)
        assert H().hm_covis_connections(self.h, len(m), p(m), int(th), p(w), p(order), p(nc)) == 0
        return w, order, nc

    def culling(self, chains, erasable, th_obs):
        off, jobs = cc.offsets(chains)
        n = int(off[-1])
        er = np.zeros(max(n, 1), np.uint8); er[:n] = [int(v) for x in erasable for v in x]
        nm = np.zeros(max(n, 1), np.int32); nr = np.zeros(max(n, 1), np.int32); red = np.zeros(max(n, 1), np.uint8)
        assert H().hm_covis_culling(self.h, len(chains), p(off), p(jobs), p(er), int(th_obs), p(nm), p(nr), p(red)) == 0
        return nm[:n], nr[:n], red[:n]

    def local_points(self, member_lists, cap):
        off, kfs = cc.offsets(member_lists)
        nj = len(member_lists)
        ids = np.full((max(nj, 1), max(cap, 1)), -1, np.int32); n_out = np.zeros(max(nj, 1), np.int32)
        rc = H().hm_covis_local_points(self.h, nj, p(off), p(kfs), int(cap), p(ids), p(n_out))
        assert rc in (0, -4), rc
        return rc, n_out[:nj], [[int(v) for v in ids[j, :min(int(n_out[j]), cap)]] for j in range(nj)]


def keyframe(mp, octave):
    """what fills a slot: the mp row and the octaves the index reads, key points inside the image, no FeatureVector"""
    n = len(mp)
    i = np.arange(n)
    kf = dict(x=(10 + i % 400).astype(np.float32), y=(10 + i // 400).astype(np.float32), octave=np.asarray(octave, np.int32), angle=np.zeros(n, np.float32),
              desc=np.zeros((n, 32), np.uint8), rays=np.tile(np.array([0, 0, 1], np.float32), (n, 1)), mp=np.asarray(mp, np.int32),
              R=np.eye(3, dtype=np.float32), t=np.zeros(3, np.float32), Ow=np.zeros(3, np.float32), median_depth=1.0,
              node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32))
    return api.make_keyframe(kf)


class DeviceBackend:
    """covis_cases.run on a KeyframeStore; queries that name a frame context run on `ctx`'s stream"""

    def __init__(self, store, ctx, max_members):
        self.st, self.ctx = store, ctx
        self.cv = api.Covisibility(store, max_members)

    def close(self):
        self.cv.close()

    def put(self, slot, mp, octave):
        K, keep = keyframe(mp, octave)
        self.st.put(int(slot), K)

    def load(self, c):
        for s, r, o in zip(c["slots"], c["rows"], c["octs"]):
            self.put(s, r, o)
        self.cv.build(c["slots"])
        return 0

    def votes(self, id_lists): return self.cv.votes(self.ctx, id_lists)
    def connections(self, members, th): return self.cv.connections(members, th)
    def culling(self, chains, erasable, th_obs): return self.cv.culling(chains, erasable, th_obs)
    def local_points(self, member_lists, cap): return self.cv.local_points(self.ctx, member_lists, cap)
