"""CPU restatement of ORBMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (src/ORBMatcher.cpp:409-539),
statement for statement, in numpy with the reference's float32 arithmetic.  The output is the key-frame feature index per frame key point (-1 = no
match), the form cms_search_by_bow returns; the caller maps it to its map point."""
import numpy as np

TH_LOW = 50
HISTO_LENGTH = 12
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def descriptor_distance(a, b):
    """ORBMatcher::DescriptorDistance: Hamming distance of two 32-byte descriptors"""
    return int(_POP[np.bitwise_xor(a, b)].sum())


def _feature_vector(fv):
    if isinstance(fv, dict):
        fv = (fv["node_id"], fv["node_off"], fv["node_feat"])
    nid, noff, nfeat = (np.asarray(a, np.int64) for a in fv)
    return [(int(nid[e]), [int(f) for f in nfeat[noff[e]:noff[e + 1]]]) for e in range(len(nid))]


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
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def search_by_bow(kf_angle, kf_desc, kf_has_mp, kf_bad, kf_fv, f_angle, f_desc, f_fv, n, nnratio, check_orientation):
    """kf_has_mp[i]: the key frame's feature i holds a map point; kf_bad None or per feature (isBad()).  fv: (node_id, node_off, node_feat) or a dict.
    Returns (kf_idx int32[n], nmatches)."""
    kf_angle = np.asarray(kf_angle, np.float32); f_angle = np.asarray(f_angle, np.float32)
    matches = np.full(n, -1, np.int32)                               # vpMapPointMatches = vector<MapPoint*>(F.N, NULL)
    nmatches = 0
    nBinsAngle = int(np.ceil(360.0 / HISTO_LENGTH))
    rotHist = [[] for _ in range(nBinsAngle)]
    factor = np.float32(1.0) / np.float32(HISTO_LENGTH)
    fvKF, fvF = _feature_vector(kf_fv), _feature_vector(f_fv)
    nnratio = np.float32(nnratio)
    ki = fi = 0
    while ki < len(fvKF) and fi < len(fvF):
        if fvKF[ki][0] == fvF[fi][0]:
            vIndicesKF, vIndicesF = fvKF[ki][1], fvF[fi][1]
            D = _POP[np.bitwise_xor(kf_desc[vIndicesKF][:, None, :], f_desc[vIndicesF][None, :, :])].sum(-1) if vIndicesKF and vIndicesF else None
            for iKF, realIdxKF in enumerate(vIndicesKF):
                if not kf_has_mp[realIdxKF]:
                    continue
                if kf_bad is not None and kf_bad[realIdxKF]:
                    continue
                bestDist1, bestIdxF, bestDist2 = 256, -1, 256
                for iF, realIdxF in enumerate(vIndicesF):
                    if matches[realIdxF] >= 0:
                        continue
                    dist = int(D[iKF, iF])                   # DescriptorDistance(dKF, dF)
                    if dist < bestDist1:
                        bestDist2 = bestDist1
                        bestDist1 = dist
                        bestIdxF = realIdxF
                    elif dist < bestDist2:
                        bestDist2 = dist
                if bestDist1 <= TH_LOW:
                    if np.float32(bestDist1) < nnratio * np.float32(bestDist2):
                        matches[bestIdxF] = realIdxKF
                        if check_orientation:
                            rot = kf_angle[realIdxKF] - f_angle[bestIdxF]
                            if rot < 0.0:
                                rot = rot + np.float32(360.0)
                            r = np.float32(rot * factor)             # round() of the reference: half away from zero
                            b = int(np.floor(np.float64(r) + 0.5)) if r >= 0 else -int(np.floor(-np.float64(r) + 0.5))
                            if b == nBinsAngle:
                                b = 0
                            assert 0 <= b < nBinsAngle
                            rotHist[b].append(bestIdxF)
                        nmatches += 1
            ki += 1
            fi += 1
        elif fvKF[ki][0] < fvF[fi][0]:
            ki = next((k for k in range(ki, len(fvKF)) if fvKF[k][0] >= fvF[fi][0]), len(fvKF))      # lower_bound
        else:
            fi = next((k for k in range(fi, len(fvF)) if fvF[k][0] >= fvKF[ki][0]), len(fvF))
    if check_orientation:
        ind1, ind2, ind3 = compute_three_maxima([len(h) for h in rotHist])
        for i in range(nBinsAngle):
            if i in (ind1, ind2, ind3):
                continue
            for j in rotHist[i]:
                matches[j] = -1
                nmatches -= 1
    return matches, nmatches
