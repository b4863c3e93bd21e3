"""CPU restatement of ORBMatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, th) (src/ORBMatcher.cpp:796-903) and of the
search half of ORBMatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint) (:1246-1363), the two projection matchers of a loop closure
(src/LoopClosing.cpp:374, :586-612), in numpy with the reference's float32 arithmetic, statement for statement: a plain sequential loop over iMP.
This is the contract of cms_kfstore_search_by_projection_sim3 and cms_kfstore_fuse_search_sim3: the device and the host build of
csrc/cms_sim3_proj_core.h are held to it bit for bit.

Conventions shared with tests/npref_sim3_search.py: R*x+t = float products and sums left to right, then (float)((double)t * 1.0 + (double)c * 1.0);
cv::norm = sqrt of the double sum of double squares, narrowed; log() on a float = libm's logf; TransformRaysToCubemap = rays_to_cubemap.
New here (one choice each, as the core header states them): scw = sqrt of the double sum of double products of row 0, narrowed once;
sRcw / scw and t / scw = one float multiply per element by (float)(1.0 / (double)scw); Ow = -Rcw.t()*tcw = per row the double sum of double
products negated, narrowed once.  PO.dot(Pn) < 0.5*dist: the double sum of double products against the double product, as the Fuse kernel has it.

`skip` != 0 <=> pMP->isBad() || spAlreadyFound.count(pMP) (:817, :1268); `taken` != 0 <=> vpMatched[idx] != NULL on entry.  One stated difference from
the reference: a ray no face takes gives u = v = -1 and is dropped by IsInImage, where the reference's assert (:836, :1287) would abort."""
import numpy as np

from npref_reloc import f32, logf, rays_to_cubemap, scale_factors      # noqa: F401  (scale_factors: for the callers)
from npref_sim3_search import _POP, _windows, distance_bounds, transform
import orc

TH_LOW = 50
INT_MAX = 2 ** 31 - 1
KEEP, BEHIND, IMAGE, DIST, ANGLE = 0, 1, 2, 3, 4


def decompose(Scw):
    """:799-803 -> dict(scw, Rcw, tcw, Ow); Scw: rows 0..2 of [sR | t] (3 x 4) or the 4 x 4"""
    S = np.asarray(Scw, np.float32).reshape(-1)[:12].reshape(3, 4)
    d = np.float64(0)
    for k in range(3):
        d = d + np.float64(S[0, k]) * np.float64(S[0, k])
    with np.errstate(all="ignore"):
        scw = f32(np.sqrt(d))                                         # const float scw = sqrt(sRcw.row(0).dot(sRcw.row(0)));
        inv = f32(np.float64(1.0) / np.float64(scw))
        Rcw = (S[:, :3] * inv).astype(np.float32)                     # cv::Mat Rcw = sRcw/scw;
        tcw = (S[:, 3] * inv).astype(np.float32)                      # cv::Mat tcw = Scw.rowRange(0,3).col(3)/scw;
        Ow = np.zeros(3, np.float32)                                  # cv::Mat Ow = -Rcw.t()*tcw;
        for r in range(3):
            s = np.float64(0)
            for k in range(3):
                s = s + np.float64(Rcw[k, r]) * np.float64(tcw[k])
            Ow[r] = f32(-1.0 * s)
    return dict(scw=scw, Rcw=Rcw, tcw=tcw, Ow=Ow)


def project(F, Scw, pos, normal, min_dist, max_dist, th, sf, bounds_scaled=0):
    """:817-860 / :1268-1312 for all points -> dict(drop, u, v (-1 unless the point reaches the distance test), dist, level, radius (-1 unless kept))"""
    sf = np.asarray(sf, np.float32)
    nlevels = len(sf)
    m = decompose(Scw)
    pos = np.asarray(pos, np.float32).reshape(-1, 3); normal = np.asarray(normal, np.float32).reshape(-1, 3)
    n = len(pos)
    with np.errstate(all="ignore"):
        pc = transform(m["Rcw"], m["tcw"], pos)                       # p3Dc = Rcw*p3Dw+tcw
        drop = np.zeros(n, np.int32)
        drop[pc[:, 2] < 0.0] = BEHIND                                 # if(p3Dc.at<float>(2)<0.0) continue;
        _, u, v = rays_to_cubemap(F, pc[:, 0], pc[:, 1], pc[:, 2])
        mx = f32(3 * F)
        inside = (u >= 0) & (u < mx) & (v >= 0) & (v < mx)            # pKF->IsInImage(u,v)
        drop[(drop == 0) & ~inside] = IMAGE
        gone = drop != 0
        u = np.where(gone, f32(-1), u).astype(np.float32); v = np.where(gone, f32(-1), v).astype(np.float32)
        PO = (pos - m["Ow"][None, :]).astype(np.float32)              # cv::Mat PO = p3Dw-Ow;
        s = np.zeros(n, np.float64)
        for k in range(3):
            s = s + PO[:, k].astype(np.float64) * PO[:, k].astype(np.float64)
        dist = np.sqrt(s).astype(np.float32)                          # const float dist = cv::norm(PO);
        minDistance, maxDistance, raw_max = distance_bounds(min_dist, max_dist, bounds_scaled)
        drop[(drop == 0) & ((dist < minDistance) | (dist > maxDistance))] = DIST
        dot = np.zeros(n, np.float64)
        for k in range(3):
            dot = dot + PO[:, k].astype(np.float64) * normal[:, k].astype(np.float64)
        drop[(drop == 0) & (dot < 0.5 * dist.astype(np.float64))] = ANGLE      # if(PO.dot(Pn)<0.5*dist) continue;
    logScale = logf(sf[1]) if nlevels > 1 else logf(f32(1.2))
    level = np.full(n, -1, np.int32); radius = np.full(n, -1, np.float32)
    raw_max = np.asarray(raw_max, np.float32)
    for i in np.flatnonzero(drop == 0):                               # pMP->PredictScale(dist, pKF)
        ratio = f32(raw_max[i] / dist[i])
        ns = int(np.ceil(f32(logf(ratio) / logScale)))
        level[i] = 0 if ns < 0 else (nlevels - 1 if ns >= nlevels else ns)
        radius[i] = f32(th) * sf[level[i]]                            # const float radius = th*pKF->mvScaleFactors[nPredictedLevel];
    return dict(drop=drop, u=u, v=v, dist=dist, level=level, radius=radius)


def _prepare(camd, sf, kf, Scw, pts, skip, th, bounds_scaled, info):
    n = len(pts["pos"])
    skip = np.zeros(n, np.uint8) if skip is None else np.asarray(skip, np.uint8)
    pr = project(camd["face"], Scw, pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], th, sf, bounds_scaled) if n else None
    drop = np.full(n, -1, np.int32)
    if n:
        drop[skip == 0] = pr["drop"][skip == 0]
    live = np.flatnonzero(drop == 0) if len(kf["kx"]) else np.zeros(0, np.int64)
    off = np.zeros(1, np.int64); idx = np.zeros(0, np.int64)
    if len(live):
        off, idx = _windows(orc.make_camera(camd), kf, pr["u"][live], pr["v"][live], pr["radius"][live])
    if info is not None:
        info.update(proj=pr, drop=drop, ncand=int(off[-1]), entries=n)
    return pr, drop, live, off, idx


def search_by_projection(camd, sf, kf, Scw, pts, skip=None, taken=None, th=10.0, bounds_scaled=0, info=None, sequential=True):
    """:796-903.  kf: dict(kx, ky, koct, kdesc); pts: dict(pos, normal, min_dist, max_dist, desc).  Returns (match int32[n points]: the key point
    vpMatched receives the point at, or -1; nmatches).  sequential=False: the same scan with the vpMatched updates switched off (for the tests'
    condition that sequencing matters).  info receives drop (-1 = skipped), ncand, entries and depth: the longest chain of points each of which had
    to wait for the one before (the rounds a parallel resolution needs)."""
    sf = np.asarray(sf, np.float32)
    pr, drop, live, off, idx = _prepare(camd, sf, kf, Scw, pts, skip, th, bounds_scaled, info)
    nk = len(kf["kx"])
    vpMatched = np.zeros(nk, bool) if taken is None else (np.asarray(taken, np.uint8) != 0)
    vpMatched = vpMatched.copy()
    match = np.full(len(drop), -1, np.int32)
    kdesc = np.asarray(kf["kdesc"], np.uint8); koct = np.asarray(kf["koct"], np.int32)
    desc = np.asarray(pts["desc"], np.uint8).reshape(-1, 32)
    nmatches = 0
    decided_at = {}                                                   # key point -> depth of the last point that had it among its free candidates
    took_at = {}                                                      # key point -> depth of the point that took it
    depth = 0
    for q, i in enumerate(live):
        vIndices = idx[off[q]:off[q + 1]]
        if len(vIndices) == 0:
            continue
        dists = _POP[np.bitwise_xor(kdesc[vIndices], desc[i][None, :])].sum(1)
        bestDist, bestIdx = 256, -1
        lv = pr["level"][i]
        mine = 1
        free = []
        for k, dist in zip(vIndices, dists):
            if vpMatched[k]:
                if int(k) in took_at and lv - 1 <= koct[k] <= lv:     # taken by an earlier point of this call: this one had to wait for it
                    mine = max(mine, took_at[int(k)] + 1)
                continue
            if koct[k] < lv - 1 or koct[k] > lv:
                continue
            free.append(int(k))
            mine = max(mine, decided_at.get(int(k), 0) + 1)
            if dist < bestDist:
                bestDist, bestIdx = int(dist), int(k)
        for k in free:
            decided_at[k] = mine
        depth = max(depth, mine)
        if bestDist <= TH_LOW:
            if sequential:
                vpMatched[bestIdx] = True
                took_at[bestIdx] = mine
            match[i] = bestIdx
            nmatches += 1
    if info is not None:
        info["depth"] = depth
    return match, nmatches


def fuse_search(camd, sf, kf, Scw, pts, skip=None, th=4.0, bounds_scaled=0, info=None):
    """:1246-1345 -> (bestIdx int32[n points] or -1, bestDist (256 where -1))"""
    sf = np.asarray(sf, np.float32)
    pr, drop, live, off, idx = _prepare(camd, sf, kf, Scw, pts, skip, th, bounds_scaled, info)
    best_idx = np.full(len(drop), -1, np.int32); best_dist = np.full(len(drop), 256, np.int32)
    kdesc = np.asarray(kf["kdesc"], np.uint8); koct = np.asarray(kf["koct"], np.int32)
    desc = np.asarray(pts["desc"], np.uint8).reshape(-1, 32)
    for q, i in enumerate(live):
        vIndices = idx[off[q]:off[q + 1]]
        if len(vIndices) == 0:
            continue
        dists = _POP[np.bitwise_xor(kdesc[vIndices], desc[i][None, :])].sum(1)
        bestDist, bestIdx = INT_MAX, -1
        lv = pr["level"][i]
        for k, dist in zip(vIndices, dists):
            if koct[k] < lv - 1 or koct[k] > lv:
                continue
            if dist < bestDist:
                bestDist, bestIdx = int(dist), int(k)
        if bestDist <= TH_LOW:
            best_idx[i] = bestIdx; best_dist[i] = bestDist
    return best_idx, best_dist
