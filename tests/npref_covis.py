"""A literal restatement of the reference's covisibility bookkeeping on Python objects: KeyFrame::UpdateConnections (src/KeyFrame.cpp:315-404),
LocalMapping::KeyFrameCulling (src/LocalMapping.cpp:561-619) with KeyFrame::SetBadFlag -> MapPoint::EraseObservation -> MapPoint::SetBadFlag
(KeyFrame.cpp:478-540, MapPoint.cpp:115-167), the votes and the max rule of Tracking::UpdateLocalKeyFrames (src/Tracking.cpp:881-928) and
Tracking::UpdateLocalPoints (:855-878).  std::map<KeyFrame*, ...> iterates in pointer order: a KeyFrame carries an `address` and every such map is
walked in ascending address.  The cases set address = member position."""


class MapPoint:
    def __init__(self, mnId):
        self.mnId = mnId
        self.mObservations = {}      # KeyFrame -> idx
        self.nObs = 0
        self.mbBad = False
        self.mnTrackReferenceForFrame = -1

    def observations(self):
        """GetObservations(): a copy, in the order a std::map<KeyFrame*, size_t> iterates"""
        return sorted(self.mObservations.items(), key=lambda kv: kv[0].address)

    def AddObservation(self, pKF, idx):      # MapPoint.cpp:105-113
        if pKF in self.mObservations:
            return
        self.mObservations[pKF] = idx
        self.nObs += 1

    def EraseObservation(self, pKF):         # MapPoint.cpp:115-136
        bBad = False
        if pKF in self.mObservations:
            self.nObs -= 1
            del self.mObservations[pKF]
            if self.nObs <= 2:
                bBad = True
        if bBad:
            self.SetBadFlag()

    def SetBadFlag(self):                    # MapPoint.cpp:150-167
        self.mbBad = True
        obs = self.observations()
        self.mObservations = {}
        for pKF, idx in obs:
            pKF.mvpMapPoints[idx] = None     # KeyFrame::EraseMapPointMatch(idx)


class KeyFrame:
    def __init__(self, mnId, address, octaves):
        self.mnId = mnId
        self.address = address
        self.octave = list(octaves)          # mvKeys[i].octave
        self.mvpMapPoints = [None] * len(self.octave)
        self.mbNotErase = False
        self.mbBad = False

    def SetBadFlag(self):                    # KeyFrame.cpp:478-497, what of it the counters can see
        if self.mnId == 0:
            return
        if self.mbNotErase:
            return                           # (mbToBeErased = true: nothing happens now)
        for pMP in self.mvpMapPoints:        # :494-496
            if pMP is not None:
                pMP.EraseObservation(self)
        self.mbBad = True


def make_map(rows, octaves, addresses=None, first_id=1):
    """rows[m][i]: the id at key point i of member m (< 0: none).  Returns (key frames in member order, {id: MapPoint}).  mnId starts at first_id:
    KeyFrameCulling and SetBadFlag skip key frame 0, which the caller of cms_covis_culling never lists."""
    kfs = [KeyFrame(first_id + m, m if addresses is None else addresses[m], octaves[m]) for m in range(len(rows))]
    points = {}
    for m, row in enumerate(rows):
        for i, id_ in enumerate(row):
            if id_ < 0:
                continue
            pMP = points.setdefault(int(id_), MapPoint(int(id_)))
            assert kfs[m] not in pMP.mObservations, "an id twice in one row"
            pMP.AddObservation(kfs[m], i)
            kfs[m].mvpMapPoints[i] = pMP
    return kfs, points


def update_connections(self, th=15):
    """KeyFrame.cpp:317-394 -> (KFcounter as {KeyFrame: weight}, mvpOrderedConnectedKeyFrames, mvOrderedWeights)"""
    KFcounter = {}
    for pMP in self.mvpMapPoints:
        if pMP is None:
            continue
        if pMP.mbBad:
            continue
        for pKFi, _ in pMP.observations():
            if pKFi.mnId == self.mnId:
                continue
            KFcounter[pKFi] = KFcounter.get(pKFi, 0) + 1
    if not KFcounter:
        return {}, [], []
    nmax = 0
    pKFmax = None
    vPairs = []
    for pKFi, w in sorted(KFcounter.items(), key=lambda kv: kv[0].address):
        if w > nmax:
            nmax = w
            pKFmax = pKFi
        if w >= th:
            vPairs.append((w, pKFi))
    if not vPairs:
        vPairs.append((nmax, pKFmax))
    vPairs.sort(key=lambda p: (p[0], p[1].address))      # sort(vPairs.begin(), vPairs.end()) on pair<int, KeyFrame*>
    lKFs, lWs = [], []
    for w, pKFi in vPairs:
        lKFs.insert(0, pKFi)                             # push_front
        lWs.insert(0, w)
    return KFcounter, lKFs, lWs


def keyframe_culling(vpLocalKeyFrames, thObs=3):
    """LocalMapping.cpp:569-618 -> [(nMPs, nRedundantObservations, redundant)] per candidate (mnId == 0 is the caller's to leave out)"""
    out = []
    for pKF in vpLocalKeyFrames:
        assert pKF.mnId != 0
        nRedundantObservations = 0
        nMPs = 0
        for i, pMP in enumerate(pKF.mvpMapPoints):
            if pMP is not None:
                if not pMP.mbBad:
                    nMPs += 1
                    if pMP.nObs > thObs:
                        scaleLevel = pKF.octave[i]
                        nObs = 0
                        for pKFi, idx in pMP.observations():
                            if pKFi is pKF:
                                continue
                            scaleLeveli = pKFi.octave[idx]
                            if scaleLeveli <= scaleLevel + 1:
                                nObs += 1
                                if nObs >= thObs:
                                    break
                        if nObs >= thObs:
                            nRedundantObservations += 1
        redundant = nRedundantObservations > 0.9 * nMPs
        if redundant:
            pKF.SetBadFlag()
        out.append((nMPs, nRedundantObservations, redundant))
    return out


def update_local_keyframes_votes(frame_points):
    """Tracking.cpp:884-928: frame_points are mCurrentFrame.mvpMapPoints' non-NULL, non-bad entries -> (keyframeCounter, pKFmax)"""
    keyframeCounter = {}
    for pMP in frame_points:
        if not pMP.mbBad:
            for pKF, _ in pMP.observations():
                keyframeCounter[pKF] = keyframeCounter.get(pKF, 0) + 1
    max_ = 0
    pKFmax = None
    for pKF, n in sorted(keyframeCounter.items(), key=lambda kv: kv[0].address):
        if pKF.mbBad:
            continue
        if n > max_:
            max_ = n
            pKFmax = pKF
    return keyframeCounter, pKFmax


def update_local_points(mvpLocalKeyFrames, frame_id=1):
    """Tracking.cpp:857-877 -> the ids of mvpLocalMapPoints"""
    mvpLocalMapPoints = []
    for pKF in mvpLocalKeyFrames:
        for pMP in pKF.mvpMapPoints:
            if pMP is None:
                continue
            if pMP.mnTrackReferenceForFrame == frame_id:
                continue
            if not pMP.mbBad:
                mvpLocalMapPoints.append(pMP)
                pMP.mnTrackReferenceForFrame = frame_id
    return [p.mnId for p in mvpLocalMapPoints]
