"""A literal numpy / Python restatement of DBoW2's vocabulary transform as ORBVocabulary uses it: the single-descriptor descent
(TemplatedVocabulary.h:1218-1259), the batch transform (:1127-1194) with BowVector::addWeight / addIfNotExist (BowVector.cpp:34-58) and
BowVector::normalize (:62-84).  std::map is a dict read in ascending key order; WordValue is a Python float (an IEEE double), math.sqrt is correctly
rounded.  An independent reading of the same lines as csrc/cms_vocab_core.h: the tests hold the two equal exactly (ids as integers, values as float64
bits).  Where the reference leaves *nid unset (a leaf above level L - levelsup) this follows DESIGN.md "ComputeBoW": nid is that leaf's id."""
import math

import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3


class Tree:
    """m_nodes as loadFromTextFile builds it: children in the order the nodes appear, word ids counting the leaves"""

    def __init__(self, t):
        self.k, self.L, self.scoring, self.weighting = t["k"], t["L"], t["scoring"], t["weighting"]
        parent = np.asarray(t["parent"])
        n = len(parent)
        # m_nodes[pid].children.push_back(nid) for nid = 1, 2, ...: per parent, the children in ascending id (a stable grouping by parent)
        self._order = 1 + np.argsort(parent[1:], kind="stable")
        self._start = np.searchsorted(parent[1:][self._order - 1], np.arange(n + 1))
        self.desc = np.asarray(t["desc"], np.uint8).reshape(n, 32)
        self.weight = np.asarray(t["weight"], np.float64)
        # m_words grows by one per line with nIsLeaf > 0
        self.word_id = np.full(n, -1, np.int64)
        lv = 1 + np.flatnonzero(np.asarray(t["is_leaf"])[1:])
        self.word_id[lv] = np.arange(len(lv))

    def children(self, nid):
        return self._order[self._start[nid]:self._start[nid + 1]]

    def is_leaf(self, nid):
        return self._start[nid] == self._start[nid + 1]


def descend(tr, feature, levelsup):
    """transform(feature, word_id, weight, nid, levelsup) -> (word_id, weight, nid)"""
    nid_level = tr.L - levelsup
    nid = 0 if nid_level <= 0 else None
    final_id = 0
    current_level = 0
    while True:
        current_level += 1
        nodes = tr.children(final_id)
        d = _POP[tr.desc[nodes] ^ feature[None, :]].sum(axis=1)
        final_id = int(nodes[0])
        best_d = int(d[0])
        for j in range(1, len(nodes)):
            if int(d[j]) < best_d:
                best_d = int(d[j])
                final_id = int(nodes[j])
        if current_level == nid_level:
            nid = final_id
        if tr.is_leaf(final_id):
            break
    if nid is None:
        nid = final_id
    return int(tr.word_id[final_id]), float(tr.weight[final_id]), nid


def must_normalize(scoring):
    """(must, norm) of the scoring object (ScoringObject.h:74-89)"""
    return scoring != 5, ("L2" if scoring == 1 else "L1")


def transform(tr, features, levelsup):
    """-> dict(word_id, word_val, node_id, node_off, node_feat)"""
    v = {}
    fv = {}
    must, norm_type = must_normalize(tr.scoring)
    add = tr.weighting in (TF, TF_IDF)
    for i_feature in range(len(features)):
        wid, w, nid = descend(tr, features[i_feature], levelsup)
        if w > 0:
            if add:
                if wid in v:
                    v[wid] += w
                else:
                    v[wid] = w
            elif wid not in v:
                v[wid] = w
            fv.setdefault(nid, []).append(i_feature)
    if add and v and not must:
        nd = float(len(v))
        for key in v:
            v[key] /= nd
    if must:
        norm = 0.0
        if norm_type == "L1":
            for key in sorted(v):
                norm += abs(v[key])
        else:
            for key in sorted(v):
                norm += v[key] * v[key]
            norm = math.sqrt(norm)
        if norm > 0.0:
            for key in v:
                v[key] /= norm
    words = sorted(v)
    nodes = sorted(fv)
    off = [0]
    feat = []
    for nid in nodes:
        feat.extend(fv[nid])
        off.append(len(feat))
    return dict(word_id=np.array(words, np.int32), word_val=np.array([v[k] for k in words], np.float64), node_id=np.array(nodes, np.int32),
                node_off=np.array(off, np.int32), node_feat=np.array(feat, np.int32))


def score_l1(v1, v2):
    """L1Scoring::score (ScoringObject.cpp:23-68) over two (word_id, word_val) pairs of ascending ids"""
    a = dict(zip((int(k) for k in v1[0]), (float(x) for x in v1[1])))
    b = dict(zip((int(k) for k in v2[0]), (float(x) for x in v2[1])))
    score = 0.0
    for key in sorted(a):
        if key in b:
            score += abs(a[key] - b[key]) - abs(a[key]) - abs(b[key])
    return -score / 2.0


def first_difference(want, got):
    """None when the two results are equal: ids as integers, values as float64 bits"""
    for key in ("word_id", "node_id", "node_off", "node_feat"):
        a, b = np.asarray(want[key]), np.asarray(got[key])
        if a.shape != b.shape or not np.array_equal(a, b):
            return "%s: %s vs %s" % (key, a[:8], b[:8])
    a, b = np.asarray(want["word_val"], np.float64), np.asarray(got["word_val"], np.float64)
    if a.shape != b.shape or not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
        bad = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64)) if a.shape == b.shape else []
        return "word_val: %d of %d differ, first %s" % (len(bad), len(a), [(int(i), float(a[i]).hex(), float(b[i]).hex()) for i in bad[:3]])
    return None
