"""A literal Python restatement of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cpp:45-314) and of the L1 score it calls (DBoW2
ScoringObject.cpp:23-68), for the key-frame database tests.  It has a real inverted file -- a list of key frames per word, appended to by add() and
searched by erase() -- and the per-key-frame fields the reference keeps (mnRelocQuery, mnRelocWords, mRelocScore, mnLoopQuery, mnLoopWords, mLoopScore);
np.float32 stands where the reference has `float`.  It shares nothing with csrc/cms_kfdb_core.h: the order of lKFsSharingWords falls out of the walk
over the inverted file here, and is a sort key there.

Two things are this project's, not the reference's: one database per group (a group is a map of its own), and mRelocScore = 0 from add() on (the
reference leaves it uninitialised until a query scores the key frame)."""
import numpy as np

RELOC, LOOP = 0, 1
COVIS = 10
f32 = np.float32


class KeyFrame:
    def __init__(self, slot, ids, vals):
        self.slot = slot
        self.mBowVec = list(zip([int(i) for i in ids], [float(v) for v in vals]))      # std::map order: ascending ids
        self.mnRelocQuery = -1; self.mnRelocWords = 0; self.mRelocScore = f32(0)
        self.mnLoopQuery = -1; self.mnLoopWords = 0; self.mLoopScore = f32(0)
        self.covis = [-1] * COVIS      # GetBestCovisibilityKeyFrames(10) as slots
        self.group = None              # the database it is in


def score(v1, v2):
    """L1Scoring::score (ScoringObject.cpp:23-68) on two ascending (id, value) lists"""
    i1, i2, e1, e2 = 0, 0, len(v1), len(v2)
    s = 0.0
    while i1 != e1 and i2 != e2:
        vi, wi = v1[i1][1], v2[i2][1]
        if v1[i1][0] == v2[i2][0]:
            s += abs(vi - wi) - abs(vi) - abs(wi)
            i1 += 1; i2 += 1
        elif v1[i1][0] < v2[i2][0]:
            while i1 != e1 and v1[i1][0] < v2[i2][0]:      # v1.lower_bound(v2_it->first)
                i1 += 1
        else:
            while i2 != e2 and v2[i2][0] < v1[i1][0]:
                i2 += 1
    return -s / 2.0


class World:
    """The slots of a store, their key frames, and one KeyFrameDatabase per group"""

    def __init__(self, K):
        self.K = K
        self.kf = [None] * K              # the key frame a slot holds a BowVector for
        self.inverted = {}                # group -> {word: [KeyFrame, ...]}  (mvInvertedFile)
        self.query_id = 0                 # F->mnId / pKF->mnId: every query is a new one

    def set_bow(self, slot, ids, vals):
        old = self.kf[slot]
        self.kf[slot] = KeyFrame(slot, ids, vals)
        if old is not None:
            self.kf[slot].covis = old.covis      # the same key frame receives its vector

    def refill(self, slot):
        if self.kf[slot] is not None and self.kf[slot].group is not None:
            self.erase([slot])
        self.kf[slot] = None

    def covisibles(self, slot, neigh):
        if self.kf[slot] is None:
            self.kf[slot] = KeyFrame(slot, [], []); self.kf[slot].no_bow = True
        self.kf[slot].covis = [int(n) for n in neigh]

    def add(self, slots, groups):      # :45-51
        for s, g in zip(slots, groups):
            kf = self.kf[s]
            inv = self.inverted.setdefault(g, {})
            for w, _ in kf.mBowVec:
                inv.setdefault(w, []).append(kf)
            kf.group = g
            kf.mRelocScore = f32(0)

    def erase(self, slots):            # :53-72
        for s in slots:
            kf = self.kf[s]
            if kf is None or kf.group is None:
                continue
            inv = self.inverted[kf.group]
            for w, _ in kf.mBowVec:
                lst = inv.get(w, [])
                for i, o in enumerate(lst):
                    if o is kf:
                        del lst[i]
                        break
            kf.group = None

    def clear(self, group):            # :74-78
        for g in list(self.inverted):
            if group < 0 or g == group:
                for lst in self.inverted[g].values():
                    for kf in lst:
                        kf.group = None
                del self.inverted[g]

    def _neighbours(self, kf):
        return [self.kf[n] for n in kf.covis if n >= 0 and self.kf[n] is not None]

    def detect_reloc(self, group, bow):      # :204-314
        self.query_id += 1
        qid = self.query_id
        inv = self.inverted.get(group, {})
        sharing = []
        for w, _ in bow:
            for kf in inv.get(w, []):
                if kf.mnRelocQuery != qid:
                    kf.mnRelocWords = 0
                    kf.mnRelocQuery = qid
                    sharing.append(kf)
                kf.mnRelocWords += 1
        scored = {}
        if not sharing:
            return [], qid, scored
        max_common = 0
        for kf in sharing:
            if kf.mnRelocWords > max_common:
                max_common = kf.mnRelocWords
        min_common = int(f32(max_common) * f32(0.8))
        score_and_match = []
        for kf in sharing:
            if kf.mnRelocWords > min_common:
                si = f32(score(bow, kf.mBowVec))
                kf.mRelocScore = si
                scored[kf.slot] = si
                score_and_match.append((si, kf))
        if not score_and_match:
            return [], qid, scored
        acc_and_match = []
        best_acc = f32(0)
        for si, kf in score_and_match:
            best_score = si
            acc = best_score
            best_kf = kf
            for kf2 in self._neighbours(kf):
                if kf2.mnRelocQuery != qid:
                    continue
                acc = f32(acc + kf2.mRelocScore)
                if kf2.mRelocScore > best_score:
                    best_kf = kf2
                    best_score = kf2.mRelocScore
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        retain = f32(f32(0.75) * best_acc)
        added, out = set(), []
        for acc, kf in acc_and_match:
            if acc > retain and id(kf) not in added:
                out.append(kf.slot)
                added.add(id(kf))
        return out, qid, scored

    def detect_loop(self, group, bow, min_score, connected):      # :81-202
        self.query_id += 1
        qid = self.query_id
        min_score = f32(min_score)
        inv = self.inverted.get(group, {})
        conn = set(id(self.kf[s]) for s in connected if self.kf[s] is not None)
        sharing = []
        for w, _ in bow:
            for kf in inv.get(w, []):
                if kf.mnLoopQuery != qid:
                    kf.mnLoopWords = 0
                    if id(kf) not in conn:
                        kf.mnLoopQuery = qid
                        sharing.append(kf)
                kf.mnLoopWords += 1
        scored = {}
        if not sharing:
            return [], qid, scored
        max_common = 0
        for kf in sharing:
            if kf.mnLoopWords > max_common:
                max_common = kf.mnLoopWords
        min_common = int(f32(max_common) * f32(0.8))
        score_and_match = []
        for kf in sharing:
            if kf.mnLoopWords > min_common:
                si = f32(score(bow, kf.mBowVec))
                kf.mLoopScore = si
                scored[kf.slot] = si
                if si >= min_score:
                    score_and_match.append((si, kf))
        if not score_and_match:
            return [], qid, scored
        acc_and_match = []
        best_acc = min_score
        for si, kf in score_and_match:
            best_score = si
            acc = si
            best_kf = kf
            for kf2 in self._neighbours(kf):
                if kf2.mnLoopQuery == qid and kf2.mnLoopWords > min_common:
                    acc = f32(acc + kf2.mLoopScore)
                    if kf2.mLoopScore > best_score:
                        best_kf = kf2
                        best_score = kf2.mLoopScore
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        retain = f32(f32(0.75) * best_acc)
        added, out = set(), []
        for acc, kf in acc_and_match:
            if acc > retain and id(kf) not in added:
                out.append(kf.slot)
                added.add(id(kf))
        return out, qid, scored

    def detect(self, job):
        """One job of kfdb_cases: (candidate slots, common words per slot int32[K], score bits per slot uint32[K] with -1.0f where not scored)"""
        q = job["query"]
        bow = list(self.kf[q[1]].mBowVec) if q[0] == "slot" else list(zip([int(i) for i in q[1]], [float(v) for v in q[2]]))
        if job["mode"] == RELOC:
            cand, qid, scored = self.detect_reloc(job["group"], bow)
            words = lambda kf: kf.mnRelocWords if kf.mnRelocQuery == qid else 0
        else:
            cand, qid, scored = self.detect_loop(job["group"], bow, job["min_score"], job["connected"])
            words = lambda kf: kf.mnLoopWords if kf.mnLoopQuery == qid else 0
        common = np.zeros(self.K, np.int32)
        sc = np.full(self.K, -1.0, np.float32)
        for s, kf in enumerate(self.kf):
            if kf is not None and kf.group is not None:
                common[s] = words(kf)
        for s, si in scored.items():
            sc[s] = si
        return list(cand), common, sc.view(np.uint32).copy()
