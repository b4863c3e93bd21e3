"""CPU restatement of ORBMatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (src/ORBMatcher.cpp:541-674), the
matcher of LoopClosing::ComputeSim3 (LoopClosing.cpp:264), statement for statement, in numpy with the reference's float32 arithmetic.  The output is
the key-frame-2 feature index per key-frame-1 key point (-1 = no match), the form cms_kfstore_search_by_bow_keyframes returns; the caller maps it to
key frame 2's map point.

feat_node1 / feat_node2 (None = the reference as it stands): what the key-frame store records per feature, the index of the FeatureVector entry that
lists it (the last one if several do, -1 = none).  With them an entry of a node's list takes part only if that node's entry is the recorded one, and a
key-frame-1 feature that holds a match is not matched again.  For every FeatureVector DBoW2 can produce (each feature in exactly one node, once) this
changes nothing; for one that lists a feature twice it makes the nodes independent of each other and the result a function of the store's contents."""
import numpy as np

from npref_bow import _POP, _feature_vector, compute_three_maxima

TH_LOW = 50
HISTO_LENGTH = 12


def feat_node_of(fv, n):
    """the store's feat_node: feature -> index of the FeatureVector entry that lists it (the last listing wins), -1 = in none"""
    fn = np.full(n, -1, np.int32)
    for e, (_, feats) in enumerate(_feature_vector(fv)):
        for f in feats:
            fn[f] = e
    return fn


def search_by_bow_kf(angle1, desc1, has_mp1, bad1, fv1, angle2, desc2, has_mp2, bad2, fv2, nnratio, check_orientation, feat_node1=None, feat_node2=None):
    """has_mp[i]: feature i holds a map point; bad None or per feature (isBad()).  fv: (node_id, node_off, node_feat) or a dict.
    Returns (idx2 int32[n1], nmatches)."""
    angle1 = np.asarray(angle1, np.float32); angle2 = np.asarray(angle2, np.float32)
    n1, n2 = len(has_mp1), len(has_mp2)
    vpMatches12 = np.full(n1, -1, np.int32)                          # vector<MapPoint*>(vpMapPoints1.size(), NULL)
    vbMatched2 = np.zeros(n2, bool)
    nBinsAngle = int(np.ceil(360.0 / HISTO_LENGTH))
    rotHist = [[] for _ in range(nBinsAngle)]
    factor = np.float32(1.0) / np.float32(HISTO_LENGTH)
    nmatches = 0
    vFeatVec1, vFeatVec2 = _feature_vector(fv1), _feature_vector(fv2)
    nnratio = np.float32(nnratio)
    f1it = f2it = 0
    while f1it < len(vFeatVec1) and f2it < len(vFeatVec2):
        if vFeatVec1[f1it][0] == vFeatVec2[f2it][0]:
            l1, l2 = vFeatVec1[f1it][1], vFeatVec2[f2it][1]
            D = _POP[np.bitwise_xor(desc1[l1][:, None, :], desc2[l2][None, :, :])].sum(-1) if l1 and l2 else None
            for i1, idx1 in enumerate(l1):
                if feat_node1 is not None and (feat_node1[idx1] != f1it or vpMatches12[idx1] >= 0):
                    continue
                if not has_mp1[idx1]:                                # if(!pMP1) continue;
                    continue
                if bad1 is not None and bad1[idx1]:                  # if(pMP1->isBad()) continue;
                    continue
                bestDist1, bestIdx2, bestDist2 = 256, -1, 256
                for i2, idx2 in enumerate(l2):
                    if feat_node2 is not None and feat_node2[idx2] != f2it:
                        continue
                    if vbMatched2[idx2] or not has_mp2[idx2]:
                        continue
                    if bad2 is not None and bad2[idx2]:
                        continue
                    dist = int(D[i1, i2])                            # DescriptorDistance(d1, d2)
                    if dist < bestDist1:
                        bestDist2 = bestDist1
                        bestDist1 = dist
                        bestIdx2 = idx2
                    elif dist < bestDist2:
                        bestDist2 = dist
                if bestDist1 < TH_LOW:
                    if np.float32(bestDist1) < nnratio * np.float32(bestDist2):
                        vpMatches12[idx1] = bestIdx2
                        vbMatched2[bestIdx2] = True
                        if check_orientation:
                            rot = angle1[idx1] - angle2[bestIdx2]
                            if rot < 0.0:
                                rot = rot + np.float32(360.0)
                            r = np.float32(rot * factor)             # round() of the reference: half away from zero
                            b = int(np.floor(np.float64(r) + 0.5)) if r >= 0 else -int(np.floor(-np.float64(r) + 0.5))
                            if b == nBinsAngle:
                                b = 0
                            assert 0 <= b < nBinsAngle
                            rotHist[b].append(idx1)
                        nmatches += 1
            f1it += 1
            f2it += 1
        elif vFeatVec1[f1it][0] < vFeatVec2[f2it][0]:
            f1it = next((k for k in range(f1it, len(vFeatVec1)) if vFeatVec1[k][0] >= vFeatVec2[f2it][0]), len(vFeatVec1))      # lower_bound
        else:
            f2it = next((k for k in range(f2it, len(vFeatVec2)) if vFeatVec2[k][0] >= vFeatVec1[f1it][0]), len(vFeatVec2))
    if check_orientation:
        ind1, ind2, ind3 = compute_three_maxima([len(h) for h in rotHist])
        for i in range(nBinsAngle):
            if i in (ind1, ind2, ind3):
                continue
            for j in rotHist[i]:
                vpMatches12[j] = -1
                nmatches -= 1
    return vpMatches12, nmatches
