"""An independent restatement of the window collection of Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:194-357) over a case of
tests/ba_window_cases.py, written the way the reference is: KeyFrame and MapPoint objects, the marks mnBALocalForKF / mnBAFixedForKF, lists that grow by
push_back, and observations iterated the way a std::map<KeyFrame*, size_t> is read in this project, by ascending member position.  No sorted key
appears here: the order of lFixedCameras is whatever the walk produces.  Doubles are made by the same IEEE operations in numpy scalars."""
import numpy as np

f32, f64 = np.float32, np.float64


class KeyFrame:
    def __init__(self, position, m, mn_id):
        self.position = position              # the member position: what orders a map of KeyFrame pointers here
        self.mnId = mn_id
        self.m = m
        self.mvpMapPoints = []                # per feature: a MapPoint or None
        self.mnBALocalForKF = -1
        self.mnBAFixedForKF = -1


class MapPoint:
    def __init__(self, id_, pos):
        self.id = id_
        self.pos = pos                        # None: the table has no row for it
        self.observations = {}                # KeyFrame -> feature index
        self.mnBALocalForKF = -1

    def GetObservations(self):
        return sorted(self.observations.items(), key=lambda kv: kv[0].position)


def build_map(c, first_member):
    pos = {int(i): c["pos"][k] for k, i in enumerate(c["pos_ids"])}
    kfs = [KeyFrame(p, m, 0 if p == first_member else p + 1) for p, m in enumerate(c["members"])]
    mps = {}
    for kf in kfs:
        for f, id_ in enumerate(kf.m["mp"]):
            id_ = int(id_)
            if id_ < 0:
                kf.mvpMapPoints.append(None)
                continue
            mp = mps.setdefault(id_, MapPoint(id_, pos.get(id_)))
            mp.observations[kf] = f
            kf.mvpMapPoints.append(mp)
    return kfs


def to_quaternion(R):
    """Eigen::Quaterniond(Matrix3d) -> (x, y, z, w)"""
    m = R.astype(f64)
    q = [f64(0)] * 4
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + f64(1.0)); q[3] = f64(0.5) * t; t = f64(0.5) / t
        q[0] = (m[2, 1] - m[1, 2]) * t; q[1] = (m[0, 2] - m[2, 0]) * t; q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + f64(1.0)); q[i] = f64(0.5) * t; t = f64(0.5) / t
        q[3] = (m[k, j] - m[j, k]) * t; q[j] = (m[j, i] + m[i, j]) * t; q[k] = (m[k, i] + m[i, k]) * t
    return q


def face_in_cubemap(F, x, y):
    """FaceInCubemap(cv::Point2f): float / int, then compared as doubles; -1 = UNKNOWN_FACE"""
    i = f64(f32(x) / f32(F)); j = f64(f32(y) / f32(F))
    if 0 <= i < 1 and 1 <= j < 2:
        return 1
    if 1 <= i < 2 and 0 <= j < 1:
        return 3
    if 1 <= i < 2 and 1 <= j < 2:
        return 0
    if 1 <= i < 2 and 2 <= j < 3:
        return 4
    if 2 <= i < 3 and 1 <= j < 2:
        return 2
    return -1


def pos_in_face(F, u):
    u = f64(u)
    return u - f64(int(u / F) * F)


def local_bundle_adjustment_window(c, local_members, first_member, F, cos_fov, inv_sigma2):
    kfs = build_map(c, first_member)
    pKF = kfs[local_members[0]]
    lLocalKeyFrames = []
    for p in local_members:                                        # :198-207: pKF, then its covisible key frames
        kfs[p].mnBALocalForKF = pKF.mnId
        lLocalKeyFrames.append(kfs[p])
    lLocalMapPoints = []
    for kf in lLocalKeyFrames:                                     # :209-225
        for mp in kf.mvpMapPoints:
            if mp is not None and mp.mnBALocalForKF != pKF.mnId:
                lLocalMapPoints.append(mp)
                mp.mnBALocalForKF = pKF.mnId
    lFixedCameras = []
    for mp in lLocalMapPoints:                                     # :227-243
        for kf, _ in mp.GetObservations():
            if kf.mnBALocalForKF != pKF.mnId and kf.mnBAFixedForKF != pKF.mnId:
                kf.mnBAFixedForKF = pKF.mnId
                lFixedCameras.append(kf)
    vertices = lLocalKeyFrames + lFixedCameras
    index = {kf: k for k, kf in enumerate(vertices)}
    poses, fixed = [], []
    for k, kf in enumerate(vertices):                              # :260-286
        poses.append([f64(v) for v in kf.m["t"]] + to_quaternion(kf.m["R"]))
        fixed.append(1 if (k >= len(lLocalKeyFrames) or kf.mnId == 0) else 0)
    points, e = [], dict(e_pose=[], e_point=[], e_obs=[], e_invsig2=[], e_face=[], e_feat=[])
    for p, mp in enumerate(lLocalMapPoints):                       # :303-356
        if mp.pos is None:
            raise LookupError("local point %d has no position" % mp.id)
        points.append([f64(v) for v in mp.pos])
        for kf, f in mp.GetObservations():
            if f32(kf.m["rays"][f, 2]) < f32(cos_fov):            # :323-325
                continue
            face = face_in_cubemap(F, kf.m["x"][f], kf.m["y"][f])
            if face < 0:
                continue
            e["e_pose"].append(index[kf]); e["e_point"].append(p); e["e_face"].append(face); e["e_feat"].append(f)
            e["e_obs"].append([pos_in_face(F, kf.m["x"][f]), pos_in_face(F, kf.m["y"][f])])
            e["e_invsig2"].append(f64(inv_sigma2[int(kf.m["oct"][f])]))
    K, P, E = len(vertices), len(lLocalMapPoints), len(e["e_pose"])
    return dict(counts=np.array([K, len(lLocalKeyFrames), P, E], np.int32), kf_member=np.array([kf.position for kf in vertices], np.int32),
                point_id=np.array([mp.id for mp in lLocalMapPoints], np.int32).reshape(P), fixed=np.array(fixed, np.uint8), poses=np.array(poses, f64).reshape(K, 7),
                points=np.array(points, f64).reshape(P, 3), e_pose=np.array(e["e_pose"], np.int32).reshape(E), e_point=np.array(e["e_point"], np.int32).reshape(E),
                e_obs=np.array(e["e_obs"], f64).reshape(E, 2), e_invsig2=np.array(e["e_invsig2"], f64).reshape(E), e_face=np.array(e["e_face"], np.int8).reshape(E),
                e_feat=np.array(e["e_feat"], np.int32).reshape(E))


def windows(c, F, cos_fov, inv_sigma2, jobs=None):
    return [local_bundle_adjustment_window(c, m, fm, F, cos_fov, inv_sigma2) for m, fm in (c["jobs"] if jobs is None else jobs)]
