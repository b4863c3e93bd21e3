"""A literal numpy restatement of the reference's map-point statistics, for tests/mpstats_cases.py:

  LocalMapping::MapPointCulling        src/LocalMapping.cpp:175-206  -> culling_verdict, Model.culling
  MapPoint::SetBadFlag                 src/MapPoint.cpp:115-136      -> Model.culling(apply)
  KeyFrame::TrackedMapPoints           src/KeyFrame.cpp:276-301      -> Model.tracked
  KeyFrame::ComputeSceneMedianDepth    src/KeyFrame.cpp:1064-1094    -> scene_median_depth, Model.median_depth
  Tracking's IncreaseVisible / Found   src/Tracking.cpp:698, :808, :829 -> Model.count

Model is the backend of mpstats_cases' runner that stands for the reference: key frames with an mp row and a pose, points with counters, and the
observation lists as the last build left them.  It refuses nothing: the refusals are the entries' own and are checked on the two real backends."""
import numpy as np

f32 = np.float32


def found_ratio(found, visible):
    """MapPoint::GetFoundRatio (MapPoint.cpp:235-239): static_cast<float>(mnFound) / mnVisible, one float division"""
    return f32(found) / f32(visible)


def culling_verdict(found, visible, first_kf, n_obs, current_kf, th_obs):
    """the chain of LocalMapping.cpp:187-204 for a point that is not bad yet: 1, 2 = SetBadFlag, 3 = erased from the list alive, 0 = stays"""
    if found_ratio(found, visible) < f32(0.25):
        return 1
    if int(current_kf) - int(first_kf) >= 2 and n_obs <= th_obs:
        return 2
    if int(current_kf) - int(first_kf) >= 3:
        return 3
    return 0


def depth(R, t, X):
    """KeyFrame.cpp:1086: Rcw2.dot(x3Dw) + zcw with Mat::dot's double sum of double products and one narrowing to float"""
    R = np.asarray(R, f32).reshape(3, 3); X = np.asarray(X, f32)
    s = np.float64(R[2, 0]) * np.float64(X[0])
    s = s + np.float64(R[2, 1]) * np.float64(X[1])
    s = s + np.float64(R[2, 2]) * np.float64(X[2])
    return f32(s + np.float64(f32(t[2])))


def depth_float_only(R, t, X):
    """the same sum in float, for the case that shows the double accumulation"""
    R = np.asarray(R, f32).reshape(3, 3); X = np.asarray(X, f32)
    return f32(f32(f32(f32(R[2, 0] * X[0]) + f32(R[2, 1] * X[1])) + f32(R[2, 2] * X[2])) + f32(t[2]))


def scene_median_depth(depths, q):
    """:1091-1093: sort, then vDepths[(size - 1) / q].  np.sort compares -0.0 and +0.0 equal, like std::sort's operator<; the entry orders -0.0f
    first, so equal values are ordered by their sign bit here (the value at the index is the same either way)"""
    d = np.asarray(depths, f32)
    if len(d) == 0:
        return f32(-1.0)
    d = d[np.lexsort((~np.signbit(d), d))]
    assert np.array_equal(d, np.sort(d))
    return d[(len(d) - 1) // q]


class Model:
    def __init__(self, K, maxf, max_points):
        self.kf = {}                   # slot -> dict(mp, R, t)
        self.median = {}
        self.pts = {}                  # id -> dict(pos, visible, found, first_kf)
        self.members = None            # slots of the last build
        self.snap = None               # their rows then
        self.max_points = max_points

    def close(self):
        pass

    # ---- the store
    def put(self, slot, mp, octave=None, R=None, t=None):
        R = np.eye(3, dtype=f32) if R is None else np.asarray(R, f32).reshape(3, 3)
        t = np.zeros(3, f32) if t is None else np.asarray(t, f32)
        self.kf[int(slot)] = dict(mp=np.array(mp, np.int32).reshape(-1), R=R, t=t)

    def update_poses(self, slots, R, t):
        for s, r, tt in zip(slots, np.asarray(R, f32).reshape(-1, 3, 3), np.asarray(t, f32).reshape(-1, 3)):
            self.kf[int(s)]["R"] = r; self.kf[int(s)]["t"] = tt

    def update_map_points(self, slot, feat, mp):
        for s, f, m in zip(slot, feat, mp):
            self.kf[int(s)]["mp"][int(f)] = int(m)

    def fetch_mp(self, slot):
        return self.kf[int(slot)]["mp"].copy()

    def build(self, slots):
        self.members = [int(s) for s in slots]
        self.snap = [self.kf[s]["mp"].copy() for s in self.members]

    def _obs(self, id_):
        """(member, feature) of the snapshot"""
        return [(m, int(f)) for m, row in enumerate(self.snap) for f in np.flatnonzero(row == id_)]

    def observations(self, id_):
        return len(self._obs(int(id_)))

    # ---- the table
    def set(self, ids, pos=None, ref=None):
        for i, id_ in enumerate(ids):
            p = self.pts.setdefault(int(id_), dict(pos=None, visible=1, found=1, first_kf=-1))      # both MapPoint constructors (MapPoint.cpp:38-41, :53-57)
            if pos is not None:
                p["pos"] = np.asarray(pos, f32).reshape(-1, 3)[i].copy()

    def erase(self, ids):
        for id_ in ids:
            self.pts.pop(int(id_), None)

    def set_stats(self, ids, first_kf=None, visible=None, found=None):
        for i, id_ in enumerate(ids):
            for k, v in (("first_kf", first_kf), ("visible", visible), ("found", found)):
                if v is not None:
                    self.pts[int(id_)][k] = int(v[i])

    def add_stats(self, ids, d_visible=None, d_found=None):
        for i, id_ in enumerate(ids):
            for k, v in (("visible", d_visible), ("found", d_found)):
                if v is not None:
                    self.pts[int(id_)][k] += int(v[i])

    def fetch_stats(self, ids):
        e = dict(visible=1, found=1, first_kf=-1)
        rows = [self.pts.get(int(i), e) for i in ids]
        return tuple(np.array([r[k] for r in rows], np.int32).reshape(-1) for k in ("visible", "found", "first_kf"))

    def count(self, which, id_lists, flags=None, count_if=1, ctx=0):
        """mnVisible++ / mnFound++ once per listed entry that names a point and passes the flag"""
        col = {1: "visible", 2: "found"}[which]
        for j, ids in enumerate(id_lists):
            for i, id_ in enumerate(ids):
                if id_ >= 0 and (flags is None or (flags[j][i] != 0) == (count_if != 0)):
                    self.pts[int(id_)][col] += 1

    def culling(self, id_lists, current_kf, th_obs=2, apply=False):
        out = []
        for ids, cur in zip(id_lists, current_kf):
            v = []
            for id_ in ids:
                p = self.pts.get(int(id_))
                v.append(4 if p is None else culling_verdict(p["found"], p["visible"], p["first_kf"], self.observations(id_), cur, th_obs))
            out.append(np.array(v, np.uint8).reshape(-1))
        if apply:
            for ids, v in zip(id_lists, out):
                for id_, vv in zip(ids, v):
                    if vv in (1, 2):      # SetBadFlag: every observer forgets the point (where its row still names it), the point is gone
                        for m, f in self._obs(int(id_)):
                            row = self.kf[self.members[m]]["mp"]
                            if row[f] == id_:
                                row[f] = -1
                        self.pts.pop(int(id_))
        return out

    def tracked(self, members, min_obs, ctx=0):
        out = []
        for m, need in zip(members, np.broadcast_to(min_obs, (len(members),))):
            n = 0
            for id_ in self.snap[int(m)]:
                if id_ >= 0 and (need <= 0 or self.observations(id_) >= need):
                    n += 1
            out.append(n)
        return np.array(out, np.int32).reshape(-1)

    def median_depth(self, slots, q=2, store=False):
        d, n = [], []
        for s in slots:
            k = self.kf[int(s)]
            z = [depth(k["R"], k["t"], self.pts[int(i)]["pos"]) for i in k["mp"] if int(i) in self.pts]
            d.append(scene_median_depth(z, q)); n.append(len(z))
            if store and z:
                self.median[int(s)] = d[-1]
        return np.array(d, f32).reshape(-1), np.array(n, np.int32).reshape(-1)
