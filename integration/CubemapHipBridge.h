// CubemapHipBridge.h -- adapters between the reference's pointer-graph types and the C-ABI of libcubemapslam_hip.so.
// Written against the reference's real headers (global-namespace Frame / KeyFrame / MapPoint / Map / Converter / CamModelGeneral);
// Not built in this repository (syntax-checked against the reference's headers by tests/test_integration_syntax.py), see integration/README.md.  Each function is the new body of the reference function it names.
#ifndef CUBEMAP_HIP_BRIDGE_H
#define CUBEMAP_HIP_BRIDGE_H
#include <list>
#include <map>
#include <set>
#include <vector>
#include <opencv2/opencv.hpp>
#include "cubemapslam_hip.h"
#include "ORBVocabulary.h"

class Frame;
class KeyFrame;
class MapPoint;
class Map;

namespace Hip {
// once, from System::System next to SetCosFovTh (System.cpp:86-89): Camera.fov of the settings file and the HIP device to use
void Configure(double camFovDeg, int device);
// cms_ctx for the camera the CamModelGeneral singleton holds (System.cpp:63-89 has set it before Tracking creates the extractors)
cms_ctx* CreateContext(const cms_orb_params& orb);

// System::CvtFisheyeToCubeMap_reverseQuery_withInterpolation (System.cpp:327-355)
void CvtFisheyeToCubeMap(cms_ctx* ctx, cv::Mat& cubemapImg, const cv::Mat& fisheyeImg);

// After Frame::Frame ran the extractor: upload nothing (cms_extract left key points + descriptors in slot 0), build the grid
// (Frame::AssignFeaturesToGrid, Frame.cpp:158-176).  Call once per frame before the searches below.
void FrameGrid(cms_ctx* ctx);

// ORBMatcher::SearchForInitialization (ORBMatcher.cpp:676-794); F2 is the frame `ctx` extracted last
int SearchForInitialization(cms_ctx* ctx, Frame& F1, Frame& F2, std::vector<cv::Point2f>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize,
                            float nnratio, bool checkOrientation);
// ORBMatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) (ORBMatcher.cpp:130-251)
int SearchByProjection(cms_ctx* ctx, Frame& CurrentFrame, const Frame& LastFrame, float th, bool checkOrientation);
// Tracking::SearchLocalPoints' two halves (Tracking.cpp:794-846): Frame::isInFrustum(pMP, 0.5) + ORBMatcher(0.8).SearchByProjection(F, vpMapPoints, th)
int SearchLocalPoints(cms_ctx* ctx, Frame& F, const std::vector<MapPoint*>& vpMapPoints, float th);
// Optimizer::PoseOptimization (Optimizer.cpp:48-190)
int PoseOptimization(Frame* pFrame);
// Optimizer::LocalBundleAdjustment (Optimizer.cpp:192-451)
void LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap);
// Optimizer::GlobalBundleAdjustemnt / BundleAdjustment (Optimizer.cpp:453-621; Tracking.cpp:514 with 20 iterations, LoopClosing.cpp:649 with 10 and
// bRobust = false): the whole map as one window, one cms_ba_optimize_global call -- optimize(nIterations), Huber(sqrt(5.99)) if bRobust, no classification;
// maps beyond the LDS solves factor their reduced camera system with the tiled LDL^T (DESIGN.md "GlobalBundleAdjustemnt").  Write-back as :577-619:
// nLoopKF == 0 through SetPose / SetWorldPos + UpdateNormalAndDepth, otherwise into mTcwGBA / mPosGBA with mnBAGlobalForKF = nLoopKF.
void GlobalBundleAdjustemnt(Map* pMap, int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true);
// The reference's g2o is single-threaded (ThirdParty/g2o/config.h:4): the same window gives the same bits every time.  SetDeterministic(true) makes every
// LocalBundleAdjustment call from then on add in a fixed order on the device (cms_ba_set_deterministic: 0.84-0.87 of the default throughput); the default adds with
// FP64 atomics and its last bits vary from run to run (DESIGN.md section 2 says what it guarantees).
void SetDeterministic(bool on);
bool GetDeterministic();

// ---- LocalMapping's per-key-frame sequence on key frames RESIDENT on the device (cms_kfstore_*).  The store maps KeyFrame* -> slot; a key frame enters
// it once (ProcessNewKeyFrame), its pose and map-point slots are refreshed where the reference changes them, and it leaves with ReleaseKeyFrame
// (KeyFrame::SetBadFlag / the end of the map).
cms_kfstore* CreateKeyFrameStore(cms_ctx* mappingCtx, int maxKeyFrames, int maxFeatures);
// LocalMapping::ProcessNewKeyFrame's device half (LocalMapping.cpp:52-117; the KeyFrame constructor's copy of the frame, KeyFrame.cpp:29-55): the frame
// `frameCtx` extracted last (slot 0 of its batch, FrameGrid already called) becomes pKF's resident copy -- key points, descriptors, key rays and grid
// device to device, mFeatVec (pKF->ComputeBoW() must have run) and the map-point slots from the host.  Returns the slot.
int ProcessNewKeyFrame(cms_kfstore* store, cms_ctx* frameCtx, KeyFrame* pKF);
void ReleaseKeyFrame(cms_kfstore* store, KeyFrame* pKF);
// the body of LocalMapping::CreateNewMapPoints (LocalMapping.cpp:209-386) for mpCurrentKeyFrame and its GetBestCovisibilityKeyFrames(20): the search,
// triangulation and every test on the device, the MapPoint bookkeeping (:359-381) here; newPoints receives what the reference pushes to
// mlpRecentAddedMapPoints.  Returns nnew.
int CreateNewMapPoints(cms_kfstore* store, KeyFrame* pCurrentKF, Map* pMap, std::vector<MapPoint*>& newPoints);
// the body of LocalMapping::SearchInNeighbors (LocalMapping.cpp:388-466): both Fuse directions as ONE device call (every set of map points uploaded
// once), then ORBMatcher::Fuse's Replace / AddObservation decisions in the reference's order (ORBMatcher.cpp:1213-1236) and the update of the
// current key frame's points and connections (:449-465)
void SearchInNeighbors(cms_kfstore* store, KeyFrame* pCurrentKF);
// after Optimizer::LocalBundleAdjustment's write-back (Optimizer.cpp:419-431): the resident copies of the local key frames get their new poses
void UpdateKeyFramePoses(cms_kfstore* store, const std::vector<KeyFrame*>& vpKFs);
// ---- Covisibility on the device (cms_covis_*): the observation index over the resident key frames of ONE map.  BuildCovisibility hands over the map's
// key frames (mpMap->GetAllKeyFrames(); bad or non-resident ones are left out), sends the entries of their map-point rows that changed since the bridge last uploaded them (ONE cms_kfstore_update_map_points) and builds the index; the
// order of vpKFs is the member order, which decides ties where the reference lets the pointer decide.  Every function below answers from the last
// BuildCovisibility of `covis`: call it after the map-point bookkeeping of the step (ProcessNewKeyFrame's AddObservation loop, Fuse) and before them.
cms_covis* CreateCovisibility(cms_kfstore* store, int maxKeyFrames);
void BuildCovisibility(cms_kfstore* store, cms_covis* covis, const std::vector<KeyFrame*>& vpKFs);
// KeyFrame::UpdateConnections (KeyFrame.cpp:315-404) for a member: KFcounter, the ordered key frames and weights from the device; AddConnection on the
// key frames that reach th = 15 (or on the one of maximal weight, :370, :377) is done here.  What remains are the assignments under mMutexConnections
// (:389-402), which touch protected members: the maintainer gives KeyFrame a three-line setter that takes this struct (integration/README.md).  The
// overload of SearchInNeighbors ends in this function instead of pKF->UpdateConnections() and returns its result.
struct Connections { std::map<KeyFrame*, int> weights; std::vector<KeyFrame*> ordered; std::vector<int> orderedWeights; };
Connections UpdateConnections(cms_kfstore* store, cms_covis* covis, KeyFrame* pKF);
Connections SearchInNeighbors(cms_kfstore* store, cms_covis* covis, KeyFrame* pCurrentKF);
// LocalMapping::KeyFrameCulling (LocalMapping.cpp:561-619) for pCurrentKF->GetVectorCovisibleKeyFrames(): the counters of the whole chain in one device
// call, cascade included, then pKF->SetBadFlag() on the redundant ones in the reference's order.  vpNotErase: the key frames whose mbNotErase is set
// (LoopClosing::SetNotErase holds them; the flag itself is protected).  Returns the key frames SetBadFlag was called on.
std::vector<KeyFrame*> KeyFrameCulling(cms_kfstore* store, cms_covis* covis, KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpNotErase = std::vector<KeyFrame*>());
// Tracking::UpdateLocalKeyFrames' votes and maximum (Tracking.cpp:884-928) and Tracking::UpdateLocalPoints (:855-878) for the frame `frameCtx` tracks:
// vpLocalKeyFrames receives the voted key frames followed by the neighbours, children and parents of :930-981 (host pointer code, unchanged), pKFmax
// the reference key frame (NULL: no votes), vpLocalMapPoints the points of the local key frames in the reference's order -- the list
// Hip::SearchLocalPoints then gathers positions for.  Bad map points of F are set to NULL like :896-899.
void UpdateLocalMap(cms_covis* covis, cms_ctx* frameCtx, Frame& F, std::vector<KeyFrame*>& vpLocalKeyFrames, KeyFrame*& pKFmax, std::vector<MapPoint*>& vpLocalMapPoints);
// ---- Map points on the device (cms_mpstore_*): MapPoint::ComputeDistinctiveDescriptors (MapPoint.cpp:243-308) and MapPoint::UpdateNormalAndDepth
// (:332-373) from the observation index, and the two per-key-frame consumers taking ids.  A map point's row is its mnId, which must be below maxPoints
// (the ids the key frames' rows and the index hold: mnId & 0x3FFFFFFF).  Observations are taken in the member order of the last BuildCovisibility, where
// the reference lets the pointer decide.
cms_mpstore* CreateMapPointStore(cms_kfstore* store, int maxPoints);
// pMP->SetWorldPos / mpRefKF as the table holds them: GetWorldPos() and GetReferenceKeyFrame() through the store's KeyFrame* -> slot book, ONE asynchronous
// cms_mpstore_set.  Bad points and points whose reference key frame is not resident are left out; returns how many were set.  Call it for the points
// CreateNewMapPoints made, and for the points a bundle adjustment moved.
int SetMapPoints(cms_mpstore* mps, const std::vector<MapPoint*>& vpMPs);
// MapPoint::SetBadFlag / Replace: the rows are empty again (one asynchronous cms_mpstore_erase)
void EraseMapPoints(cms_mpstore* mps, const std::vector<MapPoint*>& vpMPs);
// What a refresh leaves in a row: mDescriptor, mNormalVector, mfMinDistance, mfMaxDistance.  The members are protected, so MapPoint gains one setter
// that takes this struct (integration/README.md).  status: 0 done, 1 no observation in the index, 2 the reference key frame does not observe the point
// (1 and 2: the row, and the attributes here, are what they were).
struct MapPointAttributes { MapPoint* pMP; int status; cv::Mat descriptor, normal; float minDistance, maxDistance; };
// pMP->ComputeDistinctiveDescriptors() and / or pMP->UpdateNormalAndDepth() for every listed point that is set, in ONE cms_mpstore_refresh
// (what = CMS_MP_DESCRIPTOR | CMS_MP_NORMAL_DEPTH, or one of them: the reference calls UpdateNormalAndDepth alone after a bundle adjustment) and one
// cms_mpstore_fetch.  `covis`: the index after the step's BuildCovisibility.  Points that were never set are left out of the result.
std::vector<MapPointAttributes> RefreshMapPoints(cms_mpstore* mps, cms_covis* covis, const std::vector<MapPoint*>& vpMPs, int what = CMS_MP_DESCRIPTOR | CMS_MP_NORMAL_DEPTH);
// Tracking::SearchLocalPoints on rows of the table: only ids travel (cms_search_local_points_ids).  Every listed point must hold a refreshed row; the
// table's raw mfMinDistance / mfMaxDistance are used, whatever cms_set_distance_bounds_mode says.
int SearchLocalPoints(cms_ctx* ctx, cms_mpstore* mps, Frame& F, const std::vector<MapPoint*>& vpMapPoints, float th);
// LocalMapping::SearchInNeighbors on rows of the table: the Fuse search takes ids (cms_kfstore_fuse_search_sets_ids); points without a refreshed row are
// left out of the search.  Behind the reference's decisions the replaced points' rows are erased, the index is rebuilt over the members of the last
// BuildCovisibility, and the current key frame's points are set and refreshed (LocalMapping.cpp:449-463) -- `refreshed` receives their attributes --
// before UpdateConnections.
Connections SearchInNeighbors(cms_kfstore* store, cms_covis* covis, cms_mpstore* mps, KeyFrame* pCurrentKF, std::vector<MapPointAttributes>& refreshed);
// Optimizer::LocalBundleAdjustment (Optimizer.cpp:192-451) on resident data: the window (:194-357) is ONE cms_covis_local_ba_windows call over the
// index of the last BuildCovisibility and the table -- pKF and its GetVectorCovisibleKeyFrames() that are members, the key frame of mnId 0 -- then
// cms_ba_run on the arrays as they come, then the write-back of :419-450: EraseMapPointMatch / EraseObservation over (kf_member[e_pose], e_feat)
// without a search, SetPose, SetWorldPos and UpdateNormalAndDepth, and the resident copies through Hip::UpdateKeyFramePoses and Hip::SetMapPoints.
// Every local point must have been set (Hip::SetMapPoints); the table's normals and bounds are refreshed by the caller behind its next
// BuildCovisibility, which sees the erased observations.
void LocalBundleAdjustment(cms_kfstore* store, cms_covis* covis, cms_mpstore* mps, KeyFrame* pKF, bool* pbStopFlag, Map* pMap);
// ---- Map-point statistics on the device (cms_mpstore_set_stats / count / culling, cms_covis_tracked_map_points, cms_kfstore_scene_median_depth): the
// table carries mnVisible, mnFound and mnFirstKFid next to the points' rows.
// mnFirstKFid of points that are set (one asynchronous cms_mpstore_set_stats): behind Hip::SetMapPoints for the points CreateNewMapPoints made.  The
// counters need no call: a fresh row holds mnVisible = mnFound = 1 like a fresh MapPoint, and both follow through Hip::UpdateTrackStatistics.
void SetMapPointStatistics(cms_mpstore* mps, const std::vector<MapPoint*>& vpMPs);
// The statistics of one tracked frame, two asynchronous cms_mpstore_count calls on the frame context's stream: IncreaseVisible() for the local points
// Hip::SearchLocalPoints projected, inView[i] = mbTrackInView of vpLocalMapPoints[i] (Tracking.cpp:808, :829: list the frame's own points with a 1),
// and IncreaseFound() for mCurrentFrame's points that are no outliers (:698).  The host objects are counted too, so that GetFoundRatio() stays in step.
void UpdateTrackStatistics(cms_ctx* frameCtx, cms_mpstore* mps, Frame& F, const std::vector<MapPoint*>& vpLocalMapPoints, const std::vector<uint8_t>& inView);
// LocalMapping::MapPointCulling (LocalMapping.cpp:175-206): ONE cms_mpstore_culling call with apply for mlpRecentAddedMapPoints and mpCurrentKeyFrame,
// then SetBadFlag on the host objects of verdicts 1 and 2 -- the pointer graph stays in step with the rows the device has already cleared -- and the list
// handling of :184-205.  `covis`: the index of the step's BuildCovisibility (Observations() is its snapshot).  Bad points leave the list first (:187-190);
// a point the table does not hold (its mnId is beyond maxPoints, or Hip::SetMapPoints never named it) cannot be judged on the device and STAYS in the
// list with verdict 0.  Returns one verdict per point of the list as it stood after the bad ones left.  The table's book is locked for the whole
// call, so Hip::UpdateTrackStatistics on the frame thread never names a row this call has just emptied.
std::vector<uint8_t> MapPointCulling(cms_kfstore* store, cms_covis* covis, cms_mpstore* mps, std::list<MapPoint*>& lpRecentAddedMapPoints, KeyFrame* pCurrentKF);
// KeyFrame::TrackedMapPoints(minObs) (KeyFrame.cpp:276-301) of a member of the last BuildCovisibility: Tracking::NeedNewKeyFrame's nRefMatches, on the
// frame thread's stream
int TrackedMapPoints(cms_covis* covis, cms_ctx* frameCtx, KeyFrame* pKF, int minObs);
// KeyFrame::ComputeSceneMedianDepth(q) (KeyFrame.cpp:1064-1094) of a resident key frame from its row on the device and the table's positions; -1 when
// no point of the row has a position (Tracking.cpp:520 tests medianDepth < 0)
float ComputeSceneMedianDepth(cms_kfstore* store, cms_mpstore* mps, KeyFrame* pKF, int q);
// Hip::CreateNewMapPoints with the median depths of the current key frame and its neighbours taken on the device, in ONE
// cms_kfstore_scene_median_depth call with store = 1 in front of the triangulation, instead of pKF2->ComputeSceneMedianDepth(2) per neighbour
int CreateNewMapPoints(cms_kfstore* store, cms_mpstore* mps, KeyFrame* pCurrentKF, Map* pMap, std::vector<MapPoint*>& newPoints);
// ---- Tracking's SearchByBoW(KeyFrame*, Frame&, ...) (ORBMatcher.cpp:409-539) against key frames resident in `store`, on the FRAME thread: F is the frame
// `frameCtx` extracted last (slot 0 of its batch) after F.ComputeBoW().  The slot comes from the store's KeyFrame* -> slot book; a key-frame feature takes
// part where the slot's map-point entry (as ProcessNewKeyFrame / CreateNewMapPoints last wrote it) is set and GetMapPointMatches() still holds a point
// that is not bad.  Nothing runs on the store's stream (cms_kfstore_search_by_bow).  The store's book is locked from the look-up to the end of the call;
// ProcessNewKeyFrame, ReleaseKeyFrame and CreateNewMapPoints' slot updates take the same lock, so no searched slot is refilled, updated or released meanwhile.
// The body of ORBMatcher(nnratio, checkOri).SearchByBoW(pKF, F, vpMapPointMatches) in Tracking::TrackReferenceKeyFrame (Tracking.cpp:567-618).
int SearchByBoW(cms_kfstore* store, cms_ctx* frameCtx, KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches, float nnratio, bool checkOri);
// Tracking::Relocalization's candidate loop (Tracking.cpp:1019-1040) as ONE device call: vbDiscarded[i] for candidates that are bad (as the reference),
// not resident, or below 15 matches; vvpMapPointMatches[i] and nmatches[i] as SearchByBoW gives them.  The PnPsolver set-up stays with the caller.
void SearchByBoWCandidates(cms_kfstore* store, cms_ctx* frameCtx, const std::vector<KeyFrame*>& vpCandidateKFs, Frame& F,
                           std::vector<std::vector<MapPoint*> >& vvpMapPointMatches, std::vector<bool>& vbDiscarded, std::vector<int>& nmatches,
                           float nnratio, bool checkOri);
// ---- Tracking::Relocalization's guided search, ORBMatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBMatcher.cpp:253-378;
// Tracking.cpp:1101 with th 10 / ORBdist 100, :1115 with th 3 / ORBdist 64), on the FRAME thread: CurrentFrame is the frame `frameCtx` extracted last
// (slot 0 of its batch, cms_area_grid done) with the pose PnP / PoseOptimization left in mTcw.  The key frame's slot comes from the store's
// KeyFrame* -> slot book and supplies the key-point angles; a key frame that is not resident goes through cms_search_by_projection_keyframe with the
// angles from the host.  Fills CurrentFrame.mvpMapPoints like the reference and returns nmatches.  Between the two calls the PoseOptimization calls
// are Hip::PoseOptimization, and the pose comes from Hip::PnPsolver / Hip::IteratePnP below.
int SearchByProjection(cms_kfstore* store, cms_ctx* frameCtx, Frame& CurrentFrame, KeyFrame* pKF, const std::set<MapPoint*>& sAlreadyFound, float th, int ORBdist,
                       bool checkOri);
// ---- PnPsolver (include/PnPsolver.h, src/PnPsolver.cpp) with the reference's surface, for Tracking::Relocalization (Tracking.cpp:1034-1067).  The
// constructor filters and orders as :83-108 does; iterate() makes the call's draws with DUtils::Random::RandomInt -- four per iteration the loop of :184
// may need -- and runs the loop on the device.  The 2-D side (mvKeys[i].pt, mvKeyRays[i], mvLevelSigma2[octave]) is gathered on the device from the
// frame `frameCtx` extracted last (slot 0 of its batch), so F must be that frame.  When a call ends early the draws behind the accepting iteration are
// discarded: the reference's loop on the same draws, not the same rand() consumption.
class PnPsolver {
 public:
  PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches);
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991);
  cv::Mat find(cms_pnp* pnp, cms_ctx* frameCtx, std::vector<bool>& vbInliers, int& nInliers);
  cv::Mat iterate(cms_pnp* pnp, cms_ctx* frameCtx, int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

  // what IteratePnP needs of a solver
  void FillJob(cms_pnp_job& q, int nIterations);      // makes the draws
  cv::Mat TakeResult(const cms_pnp_job& q, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

 private:
  std::vector<float> mvP3Dw;                 // N x 3
  std::vector<int> mvKeyPointIndices;
  size_t mnMatches, mnKeys;
  int N, mnIterations, mnBestInliers, mRansacMinInliers, mRansacMaxIts, mRansacMinSet;
  float mRansacEpsilon, mRansacTh2, mBestTcw[12];
  std::vector<uint8_t> mvbBestInliers, mvbInliers;
  std::vector<int> mvDraws;
};
cms_pnp* CreatePnP(int maxSolvers, int maxCorrespondences, int maxHypotheses);
// One pass of Tracking.cpp:1049-1067 over the candidates that are not discarded, as ONE cms_pnp_iterate_frames call: per solver i what
// vpSolvers[i]->iterate(nIterations, bNoMore, vbInliers, nInliers) returns (an empty cv::Mat when there is no pose yet).
void IteratePnP(cms_pnp* pnp, cms_ctx* frameCtx, const std::vector<PnPsolver*>& vpSolvers, int nIterations, std::vector<cv::Mat>& vTcw,
                std::vector<bool>& vbNoMore, std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers);
// ---- LoopClosing::ComputeSim3's matcher, ORBMatcher(0.75, true).SearchByBoW(mpCurrentKF, pKF, vvpMapPointMatches[i]) (ORBMatcher.cpp:541-674), for all loop
// candidates as ONE device call on the LOOP-CLOSING thread's context `ctx`: the body of LoopClosing.cpp:251-279 up to the solver set-up.  Every candidate
// gets SetNotErase() as in the reference; vbDiscarded[i] for candidates that are bad (as the reference), not resident, or below 20 matches (all of them
// when the current key frame is not resident); vvpMapPointMatches[i][idx1] = the candidate's map point key point idx1 of pCurrentKF receives, or NULL,
// and nmatches[i], as SearchByBoW gives them.  A feature takes part where the slot's map-point entry is set and GetMapPointMatches() still holds a
// point that is not bad -- on both sides.  Nothing runs on the store's stream (cms_kfstore_search_by_bow_keyframes); the store's book is locked from
// the look-up to the end of the call, like SearchByBoWCandidates.  The caller then sets up a Hip::Sim3Solver per candidate that is not discarded.
void SearchByBoWLoopCandidates(cms_kfstore* store, cms_ctx* ctx, KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpCandidateKFs,
                               std::vector<std::vector<MapPoint*> >& vvpMapPointMatches, std::vector<bool>& vbDiscarded, std::vector<int>& nmatches,
                               float nnratio, bool checkOri);
// ---- LoopClosing::ComputeSim3's guided matcher, matcher.SearchBySim3(mpCurrentKF, pKF, vpMapPointMatches, s, R, t, 7.5) (ORBMatcher.cpp:1365-1586), for
// one or several accepted hypotheses as ONE device call on the LOOP-CLOSING thread's context `ctx`: the body of LoopClosing.cpp:312-322 behind the
// inlier copy.  Hypothesis h: candidate vpKFs[h] with s12 / R12 / t12 as Sim3Solver's GetEstimatedScale / Rotation / Translation give them and
// vvpMatches12[h] = the inlier matches of :312-317 (one entry per key point of pCurrentKF), which receives the new matches as the reference's vector
// does; vnFound[h] = what SearchBySim3 returns.  vbAlreadyMatched1 / 2 are built here with GetIndexInKeyFrame (:1390-1400); positions, the distance
// getters' values and descriptors of the map points travel with the call.  zAsWritten = true is the reference's line :1507 (the default: the
// contract is the reference's result).  Both key frames must be resident; nothing runs on the store's stream (cms_kfstore_search_by_sim3), and the
// store's book is locked from the look-up to the end of the call.  The caller goes on with Hip::OptimizeSim3 / Hip::OptimizeSim3Candidates (below).
void SearchBySim3(cms_kfstore* store, cms_ctx* ctx, KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpKFs, std::vector<std::vector<MapPoint*> >& vvpMatches12,
                  const std::vector<float>& vs12, const std::vector<cv::Mat>& vR12, const std::vector<cv::Mat>& vt12, float th, std::vector<int>& vnFound,
                  bool zAsWritten = true);
// ---- The last step of LoopClosing::ComputeSim3, matcher.SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints, 10)
// (LoopClosing.cpp:374, ORBMatcher.cpp:796-903), on the LOOP-CLOSING thread's context: the body of that statement.  spAlreadyFound, the skip flags
// (:806-807, :817) and the taken flags (vpMatched[idx] != NULL) are built here; vpMatched receives the matches as the reference's vector does; returns
// nmatches.  A key frame that is not resident goes through the reference's own matcher.  Nothing runs on the store's stream.
int SearchByProjection(cms_kfstore* store, cms_ctx* ctx, KeyFrame* pKF, const cv::Mat& Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th);
// ---- LoopClosing::SearchAndFuse (LoopClosing.cpp:586-612): matcher.Fuse(pKF, cvScw, mvpLoopMapPoints, 4, vpReplacePoints) (ORBMatcher.cpp:1246-1363) for
// every key frame of CorrectedPosesMap, as ONE cms_kfstore_fuse_search_sim3 call over the resident ones with the loop map points as one shared set,
// then the reference's own statements in the map's order and per key frame in list order: the skip test re-evaluated live at the key frame's turn
// (isBad(), GetMapPoints()), GetMapPoint(bestIdx), vpReplacePoints, AddObservation / AddMapPoint, and Replace under mMutexMapUpdate.  The search
// result of an entry depends only on geometry and descriptors, which SearchAndFuse does not change; only the skip test and what is done with bestIdx
// read pointer state, and membership of loop points in a key frame only grows meanwhile -- hence one search equals the sequential loop
// (INTEGRATION.md item 24).  A key frame that is not resident goes through the reference's own matcher.Fuse at its turn.
// vCorrectedPoses: CorrectedPosesMap in ITS order as (key frame, Converter::toCvMat(g2oScw)) -- the call site's two lines; LoopClosing.h itself is
// not pulled into this header.
void SearchAndFuse(cms_kfstore* store, cms_ctx* ctx, const std::vector<std::pair<KeyFrame*, cv::Mat> >& vCorrectedPoses, const std::vector<MapPoint*>& vpLoopMapPoints,
                   Map* pMap);
// ---- Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cpp:888-1091) behind SearchBySim3 (LoopClosing.cpp:324-326), for
// one hypothesis or for every accepted hypothesis of a pass as ONE cms_sim3_optimize call.  The start is what :324 hands g2o::Sim3: the solver's R
// (3 x 3 CV_32F), t (3 x 1 CV_32F) and s, widened as Converter::toMatrix3d / toVector3d do.  The pointer work of :941-978 is done here
// (!pMP1 || !pMP2, isBad, GetIndexInKeyFrame < 0, Rcw Xw + tcw with the reference's own cv::Mat arithmetic, mvInvLevelSigma2[octave]);
// vpMatches1[idx] becomes NULL where the reference nulls it; the return value / vnInliers[h] is the reference's.  The optimised g2oS12 comes back
// as a Sim3Estimate: g2o::Sim3(Eigen::Quaterniond(q[3], q[0], q[1], q[2]), Eigen::Vector3d(t[0], t[1], t[2]), s); it is the start when the call
// returns 0 at :1061.  jacobian = CMS_SIM3_OPT_AS_WRITTEN (default) is the reference's numeric Jacobian, CMS_SIM3_OPT_ANALYTIC the derivative.
// One stated difference: a key point in no face makes the call throw where the reference's computeError calls exit().  `ctx` supplies the face size
// and the device only; no key frame needs to be resident.
struct Sim3Estimate { double q[4], t[3], s; };      // q = x y z w
cms_sim3_opt* CreateSim3Optimizer(int maxHypotheses, int maxCorrespondences);
void OptimizeSim3Candidates(cms_sim3_opt* opt, cms_ctx* ctx, KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKF2, std::vector<std::vector<MapPoint*> >& vvpMatches1,
                            const std::vector<cv::Mat>& vR12, const std::vector<cv::Mat>& vt12, const std::vector<float>& vs12, float th2, bool bFixScale,
                            std::vector<Sim3Estimate>& vS12, std::vector<int>& vnInliers, int jacobian = CMS_SIM3_OPT_AS_WRITTEN);
int OptimizeSim3(cms_sim3_opt* opt, cms_ctx* ctx, KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, const cv::Mat& R12, const cv::Mat& t12, float s12,
                 float th2, bool bFixScale, Sim3Estimate& S12, int jacobian = CMS_SIM3_OPT_AS_WRITTEN);
// ---- Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cpp) with the reference's surface, for LoopClosing::ComputeSim3 (LoopClosing.cpp:273-345).  The
// constructor filters and orders as :66-127 does (with the reference's own cv::Mat arithmetic for Rcw Xw + tcw and its TransformRaysToCubemap);
// iterate() makes the call's draws with DUtils::Random::RandomInt -- three per iteration, for max(mRansacMaxIts - mnIterations, nIterations)
// iterations -- and runs the loop on the device.  When a call ends early the draws behind the accepting iteration are discarded: the reference's loop
// on the same draws, not the same rand() consumption.  The frame context supplies the face size and the device only.
class Sim3Solver {
 public:
  Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true);
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);
  cv::Mat find(cms_sim3* sim3, cms_ctx* frameCtx, std::vector<bool>& vbInliers12, int& nInliers);
  cv::Mat iterate(cms_sim3* sim3, cms_ctx* frameCtx, int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);
  cv::Mat GetEstimatedRotation();
  cv::Mat GetEstimatedTranslation();
  float GetEstimatedScale();

  // what IterateSim3 needs of a solver
  void FillJob(cms_sim3_job& q, int nIterations);      // makes the draws
  cv::Mat TakeResult(const cms_sim3_job& q, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

 private:
  std::vector<float> mvX3Dc1, mvX3Dc2;       // N x 3
  std::vector<float> mvnMaxError1, mvnMaxError2;
  std::vector<int> mvnIndices1;
  int N, mN1, mnIterations, mnBestInliers, mRansacMinInliers, mRansacMaxIts;
  bool mbFixScale;
  float mBestRotation[9], mBestTranslation[3], mBestScale, mBestT12[12];
  std::vector<uint8_t> mvbBestInliers, mvbInliers;
  std::vector<int> mvDraws;
};
cms_sim3* CreateSim3(int maxSolvers, int maxCorrespondences, int maxHypotheses);
// One pass of LoopClosing.cpp:287-345 over the candidates that are not discarded, as ONE cms_sim3_iterate call: per solver i what
// vpSolvers[i]->iterate(nIterations, bNoMore, vbInliers, nInliers) returns (an empty cv::Mat when there is no Sim3 yet).  The reference stops the
// pass at the first candidate OptimizeSim3 accepts; here the later candidates' iterations of that pass have run as well, which changes nothing the
// reference reads afterwards (the solvers are deleted).
void IterateSim3(cms_sim3* sim3, cms_ctx* frameCtx, const std::vector<Sim3Solver*>& vpSolvers, int nIterations, std::vector<cv::Mat>& vScm,
                 std::vector<bool>& vbNoMore, std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers);
// ---- Initializer (include/Initializer.h, src/Initializer.cpp) with the reference's surface, for Tracking::MonocularInitialization (Tracking.cpp:409
// constructs it from the first frame, :443 calls InitializeWithRays with mvIniMatches).  The constructor keeps mvKeys / mvKeyRays of the reference
// frame; InitializeWithRays makes the 8 * iterations draws with DUtils::Random::RandomInt behind SeedRandOnce(0), as :90-107 does, and runs
// FindEssential and ReconstructE on the device in one call.  Key points and key rays of CurrentFrame are taken on the device from the frame `frameCtx`
// extracted last (slot 0 of its batch), so CurrentFrame must be that frame -- the frame Hip::SearchForInitialization has just searched.  On false
// R21 and t21 are empty and vP3D / vbTriangulated are untouched, like the reference; fewer than eight matches return false.
// FillJob / TakeResult let a host with many streams put one job per stream into a single cms_init_two_view call.
class Initializer {
 public:
  Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200);
  bool InitializeWithRays(cms_init* init, cms_ctx* frameCtx, const Frame& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
                          std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated);
  bool FillJob(cms_init_job& q, const Frame& CurrentFrame, const std::vector<int>& vMatches12, bool fromFrameRow);      // makes the draws; false: fewer than 8 matches
  bool TakeResult(const cms_init_job& q, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated);

 private:
  std::vector<float> mvKeys1, mvKeyRays1, mvKeys2, mvKeyRays2, mvP3D;      // pt.x, pt.y pairs; rays x, y, z
  std::vector<int> mvMatches12, mvDraws;
  std::vector<uint8_t> mvbTriangulated;
  float mSigma;
  int mMaxIterations;
};
cms_init* CreateInitializer(int maxJobs, int maxMatches, int maxKeys1, int maxHypotheses);
// ---- ComputeBoW (src/Frame.cpp:719-726, src/KeyFrame.cpp:94-103; Tracking.cpp:570, :993, :472-473, LocalMapping.cpp:142): the vocabulary's
// transform(descriptors, mBowVec, mFeatVec, 4) on the device.  CreateVocabulary sends the tree to the device once, at start-up.  DBoW2 keeps its nodes
// protected and offers no accessor, so the tree travels through the text format: saveToTextFile into "<scratchPrefix>.<pid>.<call>.txt" (about 140 MB
// for ORBvoc.txt; the directory must be writable), read back, removed.  PRECISION: saveToTextFile prints weights with 6 significant digits.  A
// vocabulary that was itself loaded from such a text file (ORBvoc.txt: what System does) reaches the device with exactly the host's weights; one that
// was trained in this process or loaded from the binary / YAML formats does not -- save and reload it as text on the host first, or the device's
// BowVector values differ from the host's in the seventh digit.  ComputeBoW(vocab, frameCtx, F) is
// Frame::ComputeBoW for the frame `frameCtx` extracted last (slot 0 of its batch, F.N key points): it fills F.mBowVec / F.mFeatVec when mBowVec is
// empty and leaves the FeatureVector resident for cms_kfstore_search_by_bow_frames.  ComputeBoW(vocab, store, pKF) is KeyFrame::ComputeBoW for a key
// frame that entered the store (InsertKeyFrame): it fills pKF->mBowVec / mFeatVec when either is empty and leaves the slot's FeatureVector resident.
cms_vocab* CreateVocabulary(const ORBVocabulary& voc, const std::string& scratchPrefix = "cms_vocabulary_upload");
void ComputeBoW(cms_vocab* vocab, cms_ctx* frameCtx, Frame& F);
void ComputeBoW(cms_vocab* vocab, cms_kfstore* store, KeyFrame* pKF);
// ---- KeyFrameDatabase (src/KeyFrameDatabase.cpp) over the key frames resident in `store`: the database is the store's (cms_kfdb_*), so
// Tracking::Relocalization goes from Hip::ComputeBoW to Hip::SearchByBoWCandidates without fetching a BowVector.  AddToDatabase / EraseFromDatabase /
// ClearDatabase stand where the reference calls mpKeyFrameDB->add (LoopClosing.cpp:115, :145, :214), ->erase (KeyFrame.cpp:569) and ->clear
// (Tracking.cpp:1176); a key frame enters with pKF->mBowVec (as Hip::ComputeBoW or the host's ComputeBoW left it) and must be resident
// (Hip::ProcessNewKeyFrame).  Hip::ReleaseKeyFrame of a key frame that is still in the database erases it first.
// DetectRelocalizationCandidates (:204-314; Tracking.cpp:997): F is the frame `frameCtx` extracted last, after Hip::ComputeBoW(vocab, frameCtx, F) -- the
// query is the row's resident BowVector.  DetectLoopCandidates (:81-202; LoopClosing.cpp:140): pKF must be resident; its connected key frames are
// taken from pKF->GetConnectedKeyFrames().  Both hand the device every database key frame's GetBestCovisibilityKeyFrames(10) as it is at the call,
// run on frameCtx's stream (cms_kfdb_detect) and return the candidates in the reference's order.  LoopScore is the score() loop of
// LoopClosing::DetectLoop (:125-138) for pKF against its covisibles, on the store's stream.
void AddToDatabase(cms_kfstore* store, KeyFrame* pKF);
void EraseFromDatabase(cms_kfstore* store, KeyFrame* pKF);
void ClearDatabase(cms_kfstore* store);
std::vector<KeyFrame*> DetectRelocalizationCandidates(cms_kfstore* store, cms_ctx* frameCtx, Frame& F);
std::vector<KeyFrame*> DetectLoopCandidates(cms_kfstore* store, cms_ctx* frameCtx, KeyFrame* pKF, float minScore);
std::vector<double> LoopScore(cms_kfstore* store, KeyFrame* pKF, const std::vector<KeyFrame*>& vpOthers);
// ---- Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale) (src/Optimizer.cpp:623-886, call
// site LoopClosing.cpp:561) and the point loop of CorrectLoop in front of it (LoopClosing.cpp:470-500), on the device: cms_essential_graph_optimize and
// cms_sim3_correct_points (DESIGN.md "OptimizeEssentialGraph").  The pose maps are LoopClosing::KeyFrameAndPose with the estimates as Sim3Estimate
// (ToEstimates converts: this header names no g2o type).  OptimizeEssentialGraph does the pointer work of :650-825 -- one vertex per key frame that is
// not bad, in mnId order; the loop-connection edges under the minFeat = 100 rule with the (pCurKF, pLoopKF) exemption and sInsertedEdges; spanning-tree,
// loop and covisibility edges -- and writes SetPose / SetWorldPos / UpdateNormalAndDepth back under mMutexMapUpdate as :833-885 do.  The containers the
// reference orders by pointer value are walked as they are: the order of addEdge is the reference's own on the same process.
typedef std::map<KeyFrame*, Sim3Estimate> KeyFrameAndEstimate;
template <class KeyFrameAndPose>
KeyFrameAndEstimate ToEstimates(const KeyFrameAndPose& m) {
  KeyFrameAndEstimate out;
  for (typename KeyFrameAndPose::const_iterator it = m.begin(); it != m.end(); ++it) {
    Sim3Estimate e;
    e.q[0] = it->second.rotation().x(); e.q[1] = it->second.rotation().y(); e.q[2] = it->second.rotation().z(); e.q[3] = it->second.rotation().w();
    for (int i = 0; i < 3; ++i) e.t[i] = it->second.translation()[i];
    e.s = it->second.scale();
    out[it->first] = e;
  }
  return out;
}
// the handle with its capacities; the envelope's capacity follows the largest graph seen (the handle is made again when a graph needs more)
struct EssentialGraph {
  cms_ess_graph* h;
  int device, max_vertices, max_edges, max_blocks;
  EssentialGraph(int device_, int max_vertices_, int max_edges_);
  ~EssentialGraph();
  void Reserve(int vertices, int edges, long long blocks);
 private:
  EssentialGraph(const EssentialGraph&);
  EssentialGraph& operator=(const EssentialGraph&);
};
void OptimizeEssentialGraph(EssentialGraph& eg, cms_ctx* ctx, Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndEstimate& NonCorrectedSim3,
                            const KeyFrameAndEstimate& CorrectedSim3, const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections, bool bFixScale);
// LoopClosing.cpp:470-500 for every key frame of CorrectedSim3 in one launch: map points that are not bad and not yet corrected by pCurKF go through
// CorrectedSwi.map(Siw.map(P)) and get mnCorrectedByKF / mnCorrectedReference; the key frames' SetPose of :502-512 stays in CorrectLoop
void CorrectLoopPoints(cms_ctx* ctx, const KeyFrameAndEstimate& CorrectedSim3, const KeyFrameAndEstimate& NonCorrectedSim3, KeyFrame* pCurKF);

}  // namespace Hip
#endif
