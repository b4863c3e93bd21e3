"""CPU restatement of ORBMatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
(src/ORBMatcher.cpp:253-378), the guided search of Tracking::Relocalization, in numpy with the reference's float32 arithmetic.

The caller hands over the LISTED map points: those of pKF->GetMapPointMatches() that are non-NULL, not bad and not in sAlreadyFound (:268-276), in
key-frame order.  `project` is :278-305 for all of them (element-wise float32 array arithmetic: every product, sum and division rounds once, in the
reference's order); `search_by_projection_kf` is the loop itself, sequential, in list order.  Of the oracle only GetFeaturesInArea (the 41 unfolding
cases and their candidate order) and the camera's cosFovTh are used.

cv::Mat arithmetic is taken as the oracle documents it for the sibling overloads (oracle/orc_track.cpp): Rcw*x3Dw+tcw = float products and sums
left to right, then (float)((double)t * 1.0 + (double)tcw * 1.0); -Rcw.t()*tcw = double sum of double products, one rounding (transposed operand);
x3Dw-Ow float; cv::norm = sqrt of the double sum of double squares, narrowed; log() on a float = libm's logf."""
import ctypes as C
import ctypes.util

import numpy as np

import orc

HISTO_LENGTH = 12
DROP_NONE, DROP_FOV, DROP_FACE, DROP_DIST = 0, 1, 2, 3
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]
f32 = np.float32


def logf(x):
    return f32(_libm.logf(float(x)))


def scale_factors(scale_factor=1.2, nlevels=8):
    """ORBextractor's mvScaleFactor: float products, level after level"""
    sf = [f32(1.0)]
    for _ in range(1, nlevels):
        sf.append(f32(sf[-1] * f32(scale_factor)))
    return np.array(sf, np.float32)


def cos_fov_th(camd):
    """CamModelGeneral::GetCosFovTh()"""
    return f32(orc.lib().orc_cos_fov_th(C.byref(orc.make_camera(camd))))


def camera_centre(pose12):
    """const cv::Mat Ow = -Rcw.t()*tcw (:259)"""
    R = np.asarray(pose12[:9], np.float32).reshape(3, 3).astype(np.float64)
    t = np.asarray(pose12[9:12], np.float32).astype(np.float64)
    Ow = np.zeros(3, np.float32)
    for r in range(3):
        s = np.float64(0)
        for k in range(3):
            s = s + R[k, r] * t[k]
        Ow[r] = f32(-1.0 * s)
    return Ow


def rays_to_cubemap(F, x, y, z):
    """CamModelGeneral::TransformRaysToCubemap (src/CamModelGeneral.cpp:95-154) on float32 arrays -> (face or -1, up, vp).  fx = fy = cx = cy =
    F / 2 are double members: `_x * fx / _z + cx` is evaluated in double and narrowed on assignment; the face offsets are added in float."""
    x = np.asarray(x, np.float32); y = np.asarray(y, np.float32); z = np.asarray(z, np.float32)
    n = len(x)
    face = np.full(n, -1, np.int32); up = np.full(n, -1.0, np.float32); vp = np.full(n, -1.0, np.float32)
    todo = np.ones(n, bool)
    f = F / 2.0
    one = f32(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cases = [  # (face id, condition, local point, column / row of the face on the cross)
            (0, (z > 0) & (x / z <= one) & (x / z >= -one) & (y / z <= one) & (y / z >= -one), (x, y, z), (1, 1)),
            (2, (x > 0) & (y / x <= one) & (y / x >= -one) & (z / x <= one) & (z / x >= -one), (-z, y, x), (2, 1)),
            (1, (x < 0) & (y / (-x) <= one) & (y / (-x) >= -one) & (z / (-x) <= one) & (z / (-x) >= -one), (z, y, -x), (0, 1)),
            (4, (y > 0) & (x / y <= one) & (x / y >= -one) & (z / y <= one) & (z / y >= -one), (x, -z, y), (1, 2)),
            (3, (y < 0) & (x / (-y) <= one) & (x / (-y) >= -one) & (z / (-y) <= one) & (z / (-y) >= -one), (x, z, -y), (1, 0)),
        ]
        for fid, cond, (lx, ly, lz), (col, row) in cases:
            sel = todo & cond
            u = (lx.astype(np.float64) * f / lz.astype(np.float64) + f).astype(np.float32)
            v = (ly.astype(np.float64) * f / lz.astype(np.float64) + f).astype(np.float32)
            inside = sel & ~((u < 0) | (u >= F) | (v < 0) | (v >= F))
            if col:
                u = u + f32(col * F)
            if row:
                v = v + f32(row * F)
            face[inside] = fid; up[inside] = u[inside]; vp[inside] = v[inside]
            todo &= ~sel
    return face, up, vp


def project(F, cos_fov, pose12, pos, min_dist, max_dist, scale_factor=1.2, nlevels=8):
    """:278-302 for every listed point.  min_dist / max_dist = mfMinDistance / mfMaxDistance.  Returns dict(drop = why the point is skipped (DROP_*),
    u, v, level, zc, dist)."""
    pose12 = np.asarray(pose12, np.float32).reshape(12)
    R, t = pose12[:9], pose12[9:12]
    P = np.asarray(pos, np.float32).reshape(-1, 3)
    n = len(P)
    xc = np.zeros((n, 3), np.float32)
    for r in range(3):
        a = R[3 * r] * P[:, 0]
        a = a + R[3 * r + 1] * P[:, 1]
        a = a + R[3 * r + 2] * P[:, 2]
        xc[:, r] = (a.astype(np.float64) * 1.0 + np.float64(t[r]) * 1.0).astype(np.float32)
    Ow = camera_centre(pose12)
    drop = np.zeros(n, np.int32)
    zc = xc[:, 2]
    drop[zc < cos_fov] = DROP_FOV
    face, u, v = rays_to_cubemap(F, xc[:, 0], xc[:, 1], xc[:, 2])
    drop[(drop == 0) & (face < 0)] = DROP_FACE
    PO = P - Ow[None, :]
    s = np.zeros(n, np.float64)
    for k in range(3):
        s = s + PO[:, k].astype(np.float64) * PO[:, k].astype(np.float64)
    dist = np.sqrt(s).astype(np.float32)
    maxDistance = f32(1.2) * np.asarray(max_dist, np.float32)          # MapPoint::GetMaxDistanceInvariance
    minDistance = f32(0.8) * np.asarray(min_dist, np.float32)
    drop[(drop == 0) & ((dist < minDistance) | (dist > maxDistance))] = DROP_DIST
    logScale = logf(f32(scale_factor))                                 # Frame::mfLogScaleFactor
    level = np.full(n, -1, np.int32)
    for i in np.flatnonzero(drop == 0):                                # MapPoint::PredictScale(dist3D, &CurrentFrame)
        ratio = f32(np.asarray(max_dist, np.float32)[i] / dist[i])
        ns = int(np.ceil(f32(logf(ratio) / logScale)))
        level[i] = 0 if ns < 0 else (nlevels - 1 if ns >= nlevels else ns)
    return dict(drop=drop, u=u, v=v, level=level, zc=zc, dist=dist)


def rot_bin(angle_kf, angle_cur):
    rot = f32(angle_kf) - f32(angle_cur)
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    r = f32(rot * (f32(1.0) / f32(HISTO_LENGTH)))
    b = int(np.floor(np.float64(r) + 0.5)) if r >= 0 else -int(np.floor(-np.float64(r) + 0.5))      # round(): half away from zero
    nbins = int(np.ceil(360.0 / HISTO_LENGTH))
    if b == nbins:
        b = 0
    assert 0 <= b < nbins
    return b


def compute_three_maxima(hist_sizes):
    """ORBMatcher::ComputeThreeMaxima (:905-946)"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(hist_sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def _windows(cam, kx, ky, koct, qx, qy, qr, qmin, qmax):
    """Frame::GetFeaturesInArea for all windows (orc.features_in_area; repeated with the exact size where 64 candidates per window are too few)"""
    try:
        return orc.features_in_area(cam, kx, ky, koct, qx, qy, qr, qmin, qmax)
    except AssertionError as e:
        return orc.features_in_area(cam, kx, ky, koct, qx, qy, qr, qmin, qmax, cap=int(e.args[0][0]))


def search_by_projection_kf(camd, kx, ky, koct, kangle, kdesc, sf, pose12, kf_angle, pos, min_dist, max_dist, mp_desc, kp_mp, th, orb_dist,
                            check_orientation, info=None):
    """The frame: key points kx, ky, koct, kangle, descriptors kdesc, mvScaleFactors sf.  The listed points: kf_angle = pKF->mvKeys[i].angle, pos,
    min_dist / max_dist (the raw members), mp_desc.  kp_mp: int32 per frame key point, in/out: >= 0 <=> CurrentFrame.mvpMapPoints[i] != NULL; a new
    match stores the list index.  Returns (match int32[nmp], nmatches).  info (a dict) receives what the synthetic inputs are judged by: proj,
    first_choice_taken, removed, unfolded (windows that reach over an edge of their face)."""
    F = camd["face"]
    sf = np.asarray(sf, np.float32)
    kdesc = np.asarray(kdesc, np.uint8); mp_desc = np.asarray(mp_desc, np.uint8).reshape(-1, 32)
    kangle = np.asarray(kangle, np.float32); kf_angle = np.asarray(kf_angle, np.float32)
    n = len(mp_desc)
    pr = project(F, cos_fov_th(camd), pose12, pos, min_dist, max_dist, sf[1] if len(sf) > 1 else 1.2, len(sf))
    match = np.full(n, -1, np.int32)
    nmatches = 0
    nbins = int(np.ceil(360.0 / HISTO_LENGTH))
    rotHist = [[] for _ in range(nbins)]
    # the windows do not depend on the matching state: all GetFeaturesInArea calls first
    live = np.flatnonzero(pr["drop"] == 0)
    lv = pr["level"][live]
    radius = (f32(th) * sf[lv]).astype(np.float32)
    cam = orc.make_camera(camd)
    off, idx = _windows(cam, kx, ky, koct, pr["u"][live], pr["v"][live], radius, lv - 1, lv + 1)
    entry = np.array(kp_mp, copy=True)
    first_taken = removed = 0
    # windows that reach over an edge of their face: GetFeaturesInArea unfolds them onto the neighbouring face
    u, v = pr["u"][live].astype(np.float64), pr["v"][live].astype(np.float64)
    unfolded = int(((np.floor((u - radius) / F) != np.floor((u + radius) / F)) | (np.floor((v - radius) / F) != np.floor((v + radius) / F))).sum())
    for q, i in enumerate(live):
        vIndices2 = idx[off[q]:off[q + 1]]
        if len(vIndices2) == 0:
            continue
        dists = _POP[np.bitwise_xor(kdesc[vIndices2], mp_desc[i][None, :])].sum(1)
        bestDist, bestIdx2 = 256, -1
        firstDist, firstIdx2 = 256, -1                                  # the same scan on the state the call was entered with
        for i2, dist in zip(vIndices2, dists):
            if entry[i2] < 0 and dist < firstDist:
                firstDist, firstIdx2 = int(dist), int(i2)
            if kp_mp[i2] >= 0:
                continue
            if dist < bestDist:
                bestDist, bestIdx2 = int(dist), int(i2)
        if firstIdx2 >= 0 and kp_mp[firstIdx2] >= 0:
            first_taken += 1
        if bestDist <= orb_dist:
            kp_mp[bestIdx2] = i
            match[i] = bestIdx2
            nmatches += 1
            if check_orientation:
                rotHist[rot_bin(kf_angle[i], kangle[bestIdx2])].append(bestIdx2)
    if check_orientation:
        ind1, ind2, ind3 = compute_three_maxima([len(h) for h in rotHist])
        for b in range(nbins):
            if b in (ind1, ind2, ind3):
                continue
            for i2 in rotHist[b]:
                match[kp_mp[i2]] = -1
                kp_mp[i2] = -1                                          # CurrentFrame.mvpMapPoints[...] = NULL
                nmatches -= 1
                removed += 1
    if info is not None:
        info.update(proj=pr, first_choice_taken=first_taken, removed=removed, unfolded=unfolded)
    return match, nmatches
