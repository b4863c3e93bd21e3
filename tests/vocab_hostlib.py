"""ctypes access to the host side of ComputeBoW (libcubemapslam_host.so: the ORBVocabulary mirror class, the text format of io_formats.h and the host
build of csrc/cms_vocab_core.h through host_capi.cpp's hm_vocab_* functions) for the vocabulary tests."""
import ctypes as C

import numpy as np

from hostlib import load, p

_H = None
DEVICE, HOST_CORE = 0, 1


class VocabError(RuntimeError):
    pass


def H():
    global _H
    if _H is None:
        _H = load()
        _H.hm_vocab_create.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4
        _H.hm_vocab_load.argtypes = [C.c_void_p, C.c_char_p]
        _H.hm_vocab_save.argtypes = [C.c_void_p, C.c_char_p]
        _H.hm_vocab_destroy.argtypes = [C.c_void_p]; _H.hm_vocab_destroy.restype = None
        _H.hm_vocab_info.argtypes = [C.c_void_p, C.c_void_p]
        _H.hm_vocab_arrays.argtypes = [C.c_void_p] * 5
        _H.hm_vocab_transform.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        _H.hm_vocab_compute_bow_guard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _H.hm_vocab_score.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _H.hm_vocab_descend.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return _H


def _chk(rc):
    if rc != 0:
        raise VocabError(H().hm_last_error().decode())


class HostVocabulary:
    """An ORBVocabulary of the mirror (cubemap_hot_path.h)"""

    def __init__(self, t=None, path=None):
        self.h = C.c_void_p()
        if path is not None:
            _chk(H().hm_vocab_load(C.byref(self.h), str(path).encode()))
        else:
            parent = np.ascontiguousarray(t["parent"], np.int32); leaf = np.ascontiguousarray(t["is_leaf"], np.uint8)
            desc = np.ascontiguousarray(t["desc"], np.uint8); weight = np.ascontiguousarray(t["weight"], np.float64)
            _chk(H().hm_vocab_create(C.byref(self.h), int(t["k"]), int(t["L"]), int(t["scoring"]), int(t["weighting"]), len(parent), p(parent), p(leaf), p(desc), p(weight)))

    def close(self):
        if self.h:
            H().hm_vocab_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def save(self, path):
        _chk(H().hm_vocab_save(self.h, str(path).encode()))

    def tree(self):
        info = np.zeros(6, np.int32)
        _chk(H().hm_vocab_info(self.h, p(info)))
        n = int(info[4])
        t = dict(k=int(info[0]), L=int(info[1]), scoring=int(info[2]), weighting=int(info[3]), words=int(info[5]), parent=np.zeros(n, np.int32),
                 is_leaf=np.zeros(n, np.uint8), desc=np.zeros((n, 32), np.uint8), weight=np.zeros(n, np.float64))
        _chk(H().hm_vocab_arrays(self.h, p(t["parent"]), p(t["is_leaf"]), p(t["desc"]), p(t["weight"])))
        return t

    def transform(self, desc, levelsup=4, engine=HOST_CORE):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc); cap = max(n, 1)
        d = desc if n else np.zeros((1, 32), np.uint8)
        wid = np.zeros(cap, np.int32); wval = np.zeros(cap, np.float64); nid = np.zeros(cap, np.int32); noff = np.zeros(cap + 1, np.int32); nfeat = np.zeros(cap, np.int32)
        nw, nn = C.c_int(), C.c_int()
        _chk(H().hm_vocab_transform(self.h, engine, n, p(d), int(levelsup), C.byref(nw), p(wid), p(wval), C.byref(nn), p(nid), p(noff), p(nfeat)))
        nw, nn = nw.value, nn.value
        return dict(word_id=wid[:nw].copy(), word_val=wval[:nw].copy(), node_id=nid[:nn].copy(), node_off=noff[:nn + 1].copy(), node_feat=nfeat[:int(noff[nn])].copy())

    def descend(self, desc, levelsup=4):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        word = np.zeros(n, np.int32); nid = np.zeros(n, np.int32); w = np.zeros(n, np.float64)
        _chk(H().hm_vocab_descend(self.h, n, p(desc), int(levelsup), p(word), p(nid), p(w)))
        return word, nid, w

    def compute_bow_guard(self, keyframe, desc, pre_bow, pre_fv):
        """(recomputed, len(mBowVec), len(mFeatVec)) after Frame / KeyFrame::ComputeBoW with marker entries in the vectors beforehand"""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        out = np.zeros(3, np.int32)
        _chk(H().hm_vocab_compute_bow_guard(self.h, int(keyframe), len(desc), p(desc), int(pre_bow), int(pre_fv), p(out)))
        return bool(out[0]), int(out[1]), int(out[2])

    def score(self, v1, v2):
        a = (np.ascontiguousarray(v1[0], np.int32), np.ascontiguousarray(v1[1], np.float64)); b = (np.ascontiguousarray(v2[0], np.int32), np.ascontiguousarray(v2[1], np.float64))
        pad = lambda x, dt: x if len(x) else np.zeros(1, dt)
        out = C.c_double()
        _chk(H().hm_vocab_score(self.h, len(a[0]), p(pad(a[0], np.int32)), p(pad(a[1], np.float64)), len(b[0]), p(pad(b[0], np.int32)), p(pad(b[1], np.float64)), C.byref(out)))
        return out.value
