"""ctypes access to the host build of the key-frame database core (libcubemapslam_host.so: csrc/cms_kfdb_core.h through host_capi.cpp's hm_kfdb_*
functions) for the key-frame database tests.  HostDatabase is a backend of kfdb_cases.run."""
import ctypes as C

import numpy as np

from cubemapslam_amd import api
from hostlib import load, p

_H = None


def H():
    global _H
    if _H is None:
        _H = load()
        _H.hm_kfdb_create.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _H.hm_kfdb_destroy.argtypes = [C.c_void_p]; _H.hm_kfdb_destroy.restype = None
        _H.hm_kfdb_set_bow.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _H.hm_kfdb_refill.argtypes = [C.c_void_p, C.c_int]
        _H.hm_kfdb_add.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _H.hm_kfdb_erase.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _H.hm_kfdb_clear.argtypes = [C.c_void_p, C.c_int]
        _H.hm_kfdb_set_covisibles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _H.hm_kfdb_detect.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        _H.hm_kfdb_bow_score.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _H.hm_kfdb_score.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _H.hm_kfdb_mirror.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 5
    return _H


def mirror_detect(host_vocabulary, engine, descs, covis, qdesc, loop_query, min_score, connected):
    """The mirror's KeyFrameDatabase (cubemap_hot_path.h) through one engine: (relocalisation candidates, loop candidates) as key-frame indices"""
    d = np.ascontiguousarray(np.stack(descs), np.uint8); cv = np.ascontiguousarray(covis, np.int32); q = np.ascontiguousarray(qdesc, np.uint8)
    conn = np.ascontiguousarray(connected, np.int32)
    n_kf = len(d)
    reloc = np.zeros(n_kf, np.int32); loop = np.zeros(n_kf, np.int32)
    nr, nl = C.c_int(), C.c_int()
    rc = H().hm_kfdb_mirror(host_vocabulary.h, int(engine), n_kf, d.shape[1], p(d), p(cv), len(q), p(q), int(loop_query), float(min_score), len(conn), p(conn) if len(conn) else None,
                            p(reloc), C.byref(nr), p(loop), C.byref(nl))
    assert rc == 0, H().hm_last_error().decode()
    return [int(x) for x in reloc[:nr.value]], [int(x) for x in loop[:nl.value]]


def core_score(v1, v2):
    """cms_kfdb_score_host of two (ids, values) BowVectors"""
    pad = lambda x, dt: np.ascontiguousarray(x, dt) if len(x) else np.zeros(1, dt)
    out = C.c_double()
    H().hm_kfdb_score(len(v1[0]), p(pad(v1[0], np.int32)), p(pad(v1[1], np.float64)), len(v2[0]), p(pad(v2[0], np.int32)), p(pad(v2[1], np.float64)), C.byref(out))
    return out.value


class HostDatabase:
    """CmsKfdbHost behind the calls of the C-ABI; the methods return the call's code (0, -1 = CMS_ERR_ARG, -4 = CMS_ERR_OVERFLOW)"""

    def __init__(self, K, max_features):
        self.K = K
        self.h = C.c_void_p()
        assert H().hm_kfdb_create(C.byref(self.h), K, max_features) == 0

    def close(self):
        if self.h:
            H().hm_kfdb_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_bow(self, slot, ids, vals):
        ids = np.ascontiguousarray(ids, np.int32); vals = np.ascontiguousarray(vals, np.float64)
        return H().hm_kfdb_set_bow(self.h, int(slot), len(ids), p(ids) if len(ids) else None, p(vals) if len(ids) else None)

    def refill(self, slot):
        return H().hm_kfdb_refill(self.h, int(slot))

    def covis(self, slot, neigh):
        s = np.array([slot], np.int32); n = np.ascontiguousarray(neigh, np.int32)
        return H().hm_kfdb_set_covisibles(self.h, 1, p(s), p(n))

    def add(self, slots, groups):
        s = np.ascontiguousarray(slots, np.int32); g = np.ascontiguousarray(groups, np.int32)
        return H().hm_kfdb_add(self.h, len(s), p(s), p(g))

    def erase(self, slots):
        s = np.ascontiguousarray(slots, np.int32)
        return H().hm_kfdb_erase(self.h, len(s), p(s))

    def clear(self, group):
        return H().hm_kfdb_clear(self.h, int(group))

    def detect(self, jobs, cand_cap=None):
        cap = self.K if cand_cap is None else cand_cap
        arr, keep = api.kfdb_jobs(jobs)
        nj = len(jobs)
        cand = np.full((max(nj, 1), max(cap, 1)), -1, np.int32); n_cand = np.zeros(max(nj, 1), np.int32)
        common = np.zeros((max(nj, 1), self.K), np.int32); score = np.zeros((max(nj, 1), self.K), np.float32)
        self.last_rc = H().hm_kfdb_detect(self.h, nj, arr, cap, p(cand), p(n_cand), p(common), p(score))
        self.last_n_cand = n_cand
        assert self.last_rc in (0, -4), self.last_rc
        return api.kfdb_results(nj, self.K, cap, cand, n_cand, common, score)

    def bow_score(self, slot_a, slot_b):
        a = np.ascontiguousarray(slot_a, np.int32); b = np.ascontiguousarray(slot_b, np.int32)
        out = np.zeros(max(len(a), 1), np.float64)
        assert H().hm_kfdb_bow_score(self.h, len(a), p(a), p(b), p(out)) == 0
        return out[:len(a)]


def tiny_keyframe(seed):
    """what fills a slot: two features, no FeatureVector (the database reads none of it)"""
    rng = np.random.default_rng(seed)
    kf = dict(x=np.array([20.0, 40.0], np.float32), y=np.array([30.0, 50.0], np.float32), octave=np.zeros(2, np.int32), angle=np.zeros(2, np.float32),
              desc=rng.integers(0, 256, (2, 32)).astype(np.uint8), rays=np.tile(np.array([0, 0, 1], np.float32), (2, 1)), mp=np.full(2, -1, np.int32),
              R=np.eye(3, dtype=np.float32), t=np.zeros(3, np.float32), Ow=np.zeros(3, np.float32), median_depth=1.0,
              node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32))
    return api.make_keyframe(kf)


class DeviceBackend:
    """kfdb_cases.run on a KeyframeStore"""

    def __init__(self, st, ctx):
        self.st, self.ctx = st, ctx
        self.kf = tiny_keyframe(1)

    def reset(self):
        self.st.db_clear(-1)
        self.st.db_set_covisibles(np.arange(self.st.max_keyframes), np.full((self.st.max_keyframes, 10), -1, np.int32))

    def set_bow(self, slot, ids, vals): self.st.set_bow(slot, ids, vals)
    def refill(self, slot): self.st.put(slot, self.kf[0])
    def covis(self, slot, neigh): self.st.db_set_covisibles([slot], [neigh])
    def add(self, slots, groups): self.st.db_add(slots, groups)
    def erase(self, slots): self.st.db_erase(slots)
    def clear(self, group): self.st.db_clear(group)
    def detect(self, jobs): return self.st.detect_candidates(self.ctx, jobs)
