"""CPU restatement of ORBMatcher::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, s12, R12, t12, th)
(src/ORBMatcher.cpp:1365-1586), the guided matcher of LoopClosing::ComputeSim3 (src/LoopClosing.cpp:322), in numpy with the reference's float32
arithmetic, statement for statement.  This is the contract of cms_kfstore_search_by_sim3: the device and the host build of
csrc/cms_sim3_search_core.h are held to it bit for bit.

Conventions shared with tests/npref_reloc.py: R*x+t = float products and sums left to right, then (float)((double)t * 1.0 + (double)c * 1.0);
cv::norm = sqrt of the double sum of double squares, narrowed; log() on a float = libm's logf; TransformRaysToCubemap = rays_to_cubemap.
New here (one choice each, as the core header states them): s12*R12 = one float multiply per element; (1.0/s12)*R12.t() = the scalar
1.0 / (double)s12 narrowed to float, one float multiply per element; -sR21*t12 = the double sum of double products negated, narrowed once.

vbAlreadyMatched1 / 2 come in as part of `skip` (skip != 0 <=> !pMP || vbAlreadyMatched[i] || pMP->isBad()): the pointer work of :1390-1400 is the
caller's.  One stated difference from the reference: a ray no face takes gives u = v = -1 and is dropped by IsInImage, where the reference's assert
(:1430, :1511) would abort.  z_as_written: line :1507 reads `const float z = p3Dc1.at<float>(1);`; True restates it, False takes component 2."""
import numpy as np

import orc
from npref_reloc import f32, logf, rays_to_cubemap, scale_factors      # noqa: F401  (scale_factors: for the callers)

TH_HIGH = 100
INT_MAX = 2 ** 31 - 1
KEEP, BEHIND, IMAGE, DIST = 0, 1, 2, 3
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def compose(s12, R12, t12):
    """:1377-1379 -> dict(sR12, t12, sR21, t21)"""
    s12 = f32(s12)
    R = np.asarray(R12, np.float32).reshape(3, 3)
    t = np.asarray(t12, np.float32).reshape(3)
    sR12 = (s12 * R).astype(np.float32)                               # cv::Mat sR12 = s12*R12;
    inv = f32(1.0 / np.float64(s12))                                  # cv::Mat sR21 = (1.0/s12)*R12.t();
    sR21 = (inv * R.T).astype(np.float32)
    t21 = np.zeros(3, np.float32)                                     # cv::Mat t21 = -sR21*t12;
    for r in range(3):
        s = np.float64(0)
        for k in range(3):
            s = s + np.float64(sR21[r, k]) * np.float64(t[k])
        t21[r] = f32(-1.0 * s)
    return dict(sR12=sR12, t12=t.copy(), sR21=sR21, t21=t21)


def transform(R, t, P):
    """R*x + t for every row of P"""
    R = np.asarray(R, np.float32).reshape(9); t = np.asarray(t, np.float32).reshape(3)
    P = np.asarray(P, np.float32).reshape(-1, 3)
    out = np.zeros((len(P), 3), np.float32)
    for r in range(3):
        a = R[3 * r] * P[:, 0]
        a = a + R[3 * r + 1] * P[:, 1]
        a = a + R[3 * r + 2] * P[:, 2]
        out[:, r] = (a.astype(np.float64) * 1.0 + np.float64(t[r]) * 1.0).astype(np.float32)
    return out


def distance_bounds(min_in, max_in, bounds_scaled):
    """(minDistance, maxDistance, mfMaxDistance) from what the caller hands over (cms_set_distance_bounds_mode): the raw members, or the getters'
    values, from which mfMaxDistance is recovered as the float r with 1.2f * r == bound (the smaller one where two share a bound)"""
    mn = np.asarray(min_in, np.float32); mx = np.asarray(max_in, np.float32)
    if not bounds_scaled:
        return f32(0.8) * mn, f32(1.2) * mx, mx
    r = (mx.astype(np.float64) / np.float64(f32(1.2))).astype(np.float32)
    bits = r.view(np.uint32)
    lo = (bits - np.uint32(1)).view(np.float32); hi = (bits + np.uint32(1)).view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        take_lo = (r > 0) & (f32(1.2) * lo == mx)
        take_hi = ~take_lo & (f32(1.2) * r != mx) & (f32(1.2) * hi == mx)
    return mn, mx, np.where(take_lo, lo, np.where(take_hi, hi, r)).astype(np.float32)


def project(F, pose12, sR, t, pos, min_dist, max_dist, second_as_depth=False, bounds_scaled=0, scale_factor=1.2, nlevels=8):
    """One direction for all map points of one key frame (:1416-1448 / :1497-1529): pose12 = Rw | tw of the points' own key frame, sR | t the
    similarity into the other camera.  Returns dict(drop = KEEP / BEHIND / IMAGE / DIST, u, v (-1 unless the point reaches the distance test), dist,
    raw_max, level (-1 unless kept))."""
    pose12 = np.asarray(pose12, np.float32).reshape(12)
    pa = transform(pose12[:9], pose12[9:], pos)                       # p3Dc1 = R1w*p3Dw + t1w
    pb = transform(sR, t, pa)                                         # p3Dc2 = sR21*p3Dc1 + t21
    n = len(pb)
    drop = np.zeros(n, np.int32)
    drop[pb[:, 2] < 0.0] = BEHIND                                     # if(p3Dc2.at<float>(2)<0.0) continue;
    z = pb[:, 1] if second_as_depth else pb[:, 2]                     # :1426 / :1507
    _, u, v = rays_to_cubemap(F, pb[:, 0], pb[:, 1], z)
    mx = f32(3 * F)
    inside = (u >= 0) & (u < mx) & (v >= 0) & (v < mx)                # pKF->IsInImage(u, v)
    drop[(drop == 0) & ~inside] = IMAGE
    gone = drop != 0
    u = np.where(gone, f32(-1), u).astype(np.float32); v = np.where(gone, f32(-1), v).astype(np.float32)
    s = np.zeros(n, np.float64)
    for k in range(3):
        s = s + pb[:, k].astype(np.float64) * pb[:, k].astype(np.float64)
    dist = np.sqrt(s).astype(np.float32)                              # const float dist3D = cv::norm(p3Dc2);
    minDistance, maxDistance, raw_max = distance_bounds(min_dist, max_dist, bounds_scaled)
    with np.errstate(invalid="ignore"):
        drop[(drop == 0) & ((dist < minDistance) | (dist > maxDistance))] = DIST
    logScale = logf(f32(scale_factor))
    level = np.full(n, -1, np.int32)
    for i in np.flatnonzero(drop == 0):                               # pMP->PredictScale(dist3D, pKF)
        ratio = f32(raw_max[i] / dist[i])
        ns = int(np.ceil(f32(logf(ratio) / logScale)))
        level[i] = 0 if ns < 0 else (nlevels - 1 if ns >= nlevels else ns)
    return dict(drop=drop, u=u, v=v, dist=dist, raw_max=np.asarray(raw_max, np.float32), level=level)


def _windows(cam, kf, qx, qy, qr):
    """KeyFrame::GetFeaturesInArea(u, v, radius) for all windows (no level arguments); repeated with the exact size where 64 per window are too few"""
    m1 = np.full(len(qx), -1, np.int32)
    try:
        return orc.features_in_area(cam, kf["kx"], kf["ky"], kf["koct"], qx, qy, qr, m1, m1)
    except AssertionError as e:
        return orc.features_in_area(cam, kf["kx"], kf["ky"], kf["koct"], qx, qy, qr, m1, m1, cap=int(e.args[0][0]))


def _direction(camd, sf, pose12, sR, t, mp, kf_other, th, second_as_depth, bounds_scaled, info):
    """one loop of :1406-1484 / :1487-1565 -> vnMatch"""
    n = len(mp["skip"])
    vnMatch = np.full(n, -1, np.int32)
    info.update(proj=None, ncand=0)
    if n == 0:
        return vnMatch
    pr = project(camd["face"], pose12, sR, t, mp["pos"], mp["min_dist"], mp["max_dist"], second_as_depth, bounds_scaled, sf[1] if len(sf) > 1 else 1.2, len(sf))
    info["proj"] = pr
    live = np.flatnonzero((np.asarray(mp["skip"]) == 0) & (pr["drop"] == 0))
    if len(live) == 0 or len(kf_other["kx"]) == 0:
        return vnMatch
    lv = pr["level"][live]
    radius = (f32(th) * sf[lv]).astype(np.float32)                    # const float radius = th*pKF2->mvScaleFactors[nPredictedLevel];
    off, idx = _windows(orc.make_camera(camd), kf_other, pr["u"][live], pr["v"][live], radius)
    info["ncand"] = int(off[-1])
    kdesc = np.asarray(kf_other["kdesc"], np.uint8); koct = np.asarray(kf_other["koct"], np.int32)
    mp_desc = np.asarray(mp["desc"], np.uint8).reshape(-1, 32)
    for q, i in enumerate(live):
        vIndices = idx[off[q]:off[q + 1]]
        if len(vIndices) == 0:
            continue
        dists = _POP[np.bitwise_xor(kdesc[vIndices], mp_desc[i][None, :])].sum(1)
        bestDist, bestIdx = INT_MAX, -1
        for k, dist in zip(vIndices, dists):
            if koct[k] < lv[q] - 1 or koct[k] > lv[q]:
                continue
            if dist < bestDist:
                bestDist, bestIdx = int(dist), int(k)
        if bestDist <= TH_HIGH:
            vnMatch[i] = bestIdx
    return vnMatch


def search_by_sim3(camd, sf, kf1, kf2, s12, R12, t12, mp1, mp2, th=7.5, z_as_written=True, bounds_scaled=0, info=None):
    """kf1 / kf2: dict(kx, ky, koct, kdesc, pose12 = Rcw | tcw).  mp1 / mp2: per key point of that key frame dict(skip, pos, min_dist, max_dist, desc).
    Returns (idx2 int32[n1]: the key point of key frame 2 whose map point key point i1 of key frame 1 receives, or -1; nFound).  info (a dict)
    receives vnMatch1, vnMatch2, the two projections and the number of window candidates of both directions."""
    sf = np.asarray(sf, np.float32)
    m = compose(s12, R12, t12)
    i1, i2 = {}, {}
    vnMatch1 = _direction(camd, sf, kf1["pose12"], m["sR21"], m["t21"], mp1, kf2, th, False, bounds_scaled, i1)
    vnMatch2 = _direction(camd, sf, kf2["pose12"], m["sR12"], m["t12"], mp2, kf1, th, bool(z_as_written), bounds_scaled, i2)
    idx2 = np.full(len(vnMatch1), -1, np.int32)
    nFound = 0
    for a in range(len(vnMatch1)):                                    # :1567-1583
        b = vnMatch1[a]
        if b >= 0 and vnMatch2[b] == a:
            idx2[a] = b
            nFound += 1
    if info is not None:
        info.update(vnMatch1=vnMatch1, vnMatch2=vnMatch2, proj1=i1["proj"], proj2=i2["proj"], ncand=i1["ncand"] + i2["ncand"], entries=len(vnMatch1) + len(vnMatch2))
    return idx2, nFound
