// cubemap_hot_path.h -- host-side C++ mirror of the reference interfaces on the hot path, implemented on top of the
// C-ABI of libcubemapslam_hip.so (include/cubemapslam_hip.h).  Same class / method names, argument meaning and error
// behaviour as the reference so Tracking / LocalMapping style call sites read unchanged:
//
//   CamModelGeneral::GetCamera()->SetCamParams(...)                 include/CamModelGeneral.h:100-108, src/System.cpp:63-89
//   System::CreateUndistortRectifyMap / CvtFisheyeToCubeMap_reverseQuery_withInterpolation
//                                                                   include/System.h:104-107, src/System.cpp:301-355
//   ORBextractor(int,float,int,int,int) / operator()(image, mask, keypoints, descriptors) / Get* accessors
//                                                                   include/ORBExtractor.h:55-90, src/ORBExtractor.cpp:838-926
//   ORBMatcher(nnratio, checkOri) / DescriptorDistance / SearchByProjection(CurrentFrame, LastFrame, th, mono)
//                                                                   include/ORBMatcher.h:46-84, src/ORBMatcher.cpp:130-251,951-967
//   Optimizer::LocalBundleAdjustment(...)                           include/Optimizer.h:50, src/Optimizer.cpp:192-451
//   Optimizer::GlobalBundleAdjustemnt(...)                          include/Optimizer.h, src/Optimizer.cpp:453-621
//   ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) loadFromTextFile / saveToTextFile / transform / score
//                                                                   include/ORBVocabulary.h, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h
//
// The pointer-graph types the reference passes around (Frame, KeyFrame, MapPoint, Map) are out of scope (SURVEY.md
// section 2); the two methods that take them receive plain views instead (FrameView, LocalBAWindow) holding exactly the
// fields those methods read.
#ifndef CMS_CUBEMAP_HOT_PATH_H
#define CMS_CUBEMAP_HOT_PATH_H
#include <functional>
#include <list>
#include <map>
#include <string>
#include <set>
#include <vector>
#include "cubemapslam_hip.h"
#include "io_formats.h"
#include "mini_cv.h"

namespace CubemapSLAM {

// DBoW2::BowVector (std::map<WordId, WordValue>) and DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>) in std::map order
typedef std::vector<std::pair<unsigned, double>> BowVector;
typedef std::vector<std::pair<unsigned, std::vector<unsigned>>> FeatureVector;

// ORBVocabulary under the reference's names.  loadFromTextFile reads ORBvoc.txt's format (io_formats.h; false with the reason in error() for a file
// the loader refuses -- unlike the reference it skips empty lines and checks the tree), saveToTextFile writes the reference's bytes.  transform runs
// on the shared context's device (engine DEVICE, the default: cms_vocab_transform) or through the host build of the same core (engine HOST_CORE:
// csrc/cms_vocab_core.h, the definition of record, no GPU needed).  score is L1Scoring::score (ScoringObject.cpp:23-68); the other scoring types
// throw std::runtime_error.
class ORBVocabulary {
 public:
  enum Engine { DEVICE = 0, HOST_CORE = 1 };
  ORBVocabulary();
  ~ORBVocabulary();
  ORBVocabulary(const ORBVocabulary&) = delete;
  ORBVocabulary& operator=(const ORBVocabulary&) = delete;
  bool loadFromTextFile(const std::string& filename);
  void saveToTextFile(const std::string& filename) const;
  bool setTree(const VocabularyText& tree);      // the same checks as loadFromTextFile, from arrays
  bool empty() const;
  unsigned size() const;                         // number of words
  void transform(const std::vector<cv::Mat>& features, BowVector& v, FeatureVector& fv, int levelsup) const;
  double score(const BowVector& v1, const BowVector& v2) const;
  const VocabularyText& tree() const;
  const std::string& error() const { return error_; }
  cms_vocab* deviceHandle() const;               // created on first use on the shared context's device (device 0)
  mutable Engine engine = DEVICE;

 private:
  struct Impl;
  Impl* impl_;
  std::string error_;
};

class CamModelGeneral {
 public:
  enum eFace { UNKNOWN_FACE = -1, FRONT_FACE = 0, LEFT_FACE = 1, RIGHT_FACE = 2, UPPER_FACE = 3, LOWER_FACE = 4 };
  static CamModelGeneral* GetCamera();
  // same argument order as the reference overload used by System (CamModelGeneral.h:105-108); poly / invpoly zero padded
  void SetCamParams(const double cdeu0v0[5], const std::vector<double>& poly, const std::vector<double>& invpoly, double Iw,
                    double Ih, double fx, double fy, double cx, double cy, double width, double height, double camFov);
  int GetCubeFaceWidth() const { return cam_.face; }
  int GetCubeFaceHeight() const { return cam_.face; }
  int GetFisheyeWidth() const { return cam_.Iw; }
  int GetFisheyeHeight() const { return cam_.Ih; }
  double Get_fx() const { return cam_.face / 2.0; }
  float GetCosFovTh() const { return cosFovTh_; }
  eFace FaceInCubemap(const cv::Point2f& pixel) const;                          // CamModelGeneral.h:445-456
  void GetPosInFace(double& u, double& v, double uCubemap, double vCubemap) const;  // CamModelGeneral.h:204-209
  const cms_camera& params() const { return cam_; }
  bool configured() const { return configured_; }

 private:
  cms_camera cam_{};
  float cosFovTh_ = 0;
  bool configured_ = false;
};

// Owner of the device context shared by the remap entry point and the extractor (one per process, like the reference's
// camera singleton + System instance).  Throws std::runtime_error when the HIP library cannot create a context.
cms_ctx* SharedContext(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST);

// one key frame of the trajectory output: KeyFrame::mTimeStamp and its world->camera pose (KeyFrame::GetPose(), 4x4 CV_32F)
struct TrajectoryKeyFrame { double mTimeStamp; cv::Mat Tcw; bool bad = false; };

class System {
 public:
  // System.cpp:238-268: one line per (non-bad) key frame, "ts tx ty tz qx qy qz qw" with the camera centre -R^T t and the
  // quaternion of R^T through float, fixed notation, 6 digits for the time stamp and 7 for the rest.  The caller passes
  // the key frames already sorted by id (the reference sorts with KeyFrame::lId).
  static void SaveKeyFrameTrajectoryTUM(const std::string& filename, const std::vector<TrajectoryKeyFrame>& vpKFs);
  void CreateUndistortRectifyMap();  // builds the LUT on the device (inside the shared context)
  void CvtFisheyeToCubeMap_reverseQuery_withInterpolation(cv::Mat& cubemapImg, const cv::Mat& fisheyeImg, int interpolation,
                                                          int borderType = cv::BORDER_CONSTANT,
                                                          const cv::Scalar& borderValue = cv::Scalar());
};

class ORBextractor {
 public:
  ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST);
  // image: CV_8UC1 3F x 3F cubemap; mask: CV_8UC1 non-empty (assert in the reference, ORBExtractor.cpp:845-848);
  // empty image -> silent return (ORBExtractor.cpp:841).
  void operator()(cv::InputArray image, cv::InputArray mask, std::vector<cv::KeyPoint>& keypoints, cv::OutputArray descriptors);
  int GetLevels() const { return nlevels; }
  float GetScaleFactor() const { return (float)scaleFactor; }
  std::vector<float> GetScaleFactors() const { return mvScaleFactor; }
  std::vector<float> GetInverseScaleFactors() const { return mvInvScaleFactor; }
  std::vector<float> GetScaleSigmaSquares() const { return mvLevelSigma2; }
  std::vector<float> GetInverseScaleSigmaSquares() const { return mvInvLevelSigma2; }

  // ORBExtractor.h:89-90.  The reference keeps the (19-px padded) level images of the last call here; no stage of the hot path reads
  // them afterwards, so the mirror only fetches them from the device when a caller sets mbKeepImagePyramid -- level l is the
  // cvRound(W / scale_l)^2 image without the border frame ("19-px REFLECT_101 frame").
  std::vector<cv::Mat> mvImagePyramid;
  std::vector<cv::Mat> mvMaskPyramid;      // resized and never filled in the reference either (ORBExtractor.cpp:405)
  bool mbKeepImagePyramid = false;

 protected:
  int nfeatures; double scaleFactor; int nlevels, iniThFAST, minThFAST;
  std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
  cms_ctx* ctx_ = nullptr;
  const uint8_t* last_mask_ = nullptr;
};

// What ORBMatcher::SearchByProjection(Frame&, const Frame&, th, mono) reads from a Frame (Frame.h): key points,
// descriptors, the map-point slot per key point (>=0 = id of the assigned map point) and, for the last frame, the
// projection of each of its map points into the current frame (u, v in cubemap pixels, <0 = not visible).
struct FrameView {
  std::vector<cv::KeyPoint> mvKeys;
  cv::Mat mDescriptors;                 // N x 32 CV_8U
  std::vector<long> mvpMapPoints;       // -1 = none
  std::vector<uint8_t> mvbOutlier;
  std::vector<cv::Point2f> projInCurrent;  // last frame only: where map point i projects in the current frame
  std::vector<float> mvScaleFactors;
  cv::Mat mTcw;                         // 4x4 CV_32F (Frame::SetPose): SearchLocalPoints, and SearchByProjection's device path
  // last frame only, optional: world position and descriptor of the map point behind key point i (MapPoint::GetWorldPos / GetDescriptor).
  // When given (and CurrentFrame.mTcw is set) SearchByProjection projects on the device instead of reading projInCurrent.
  std::vector<cv::Vec3f> mvMapPointPos;
  cv::Mat mMapPointDescriptors;         // N x 32 CV_8U
  std::vector<std::pair<unsigned, std::vector<unsigned>>> mFeatVec;   // Frame::ComputeBoW: ascending node id (SearchByBoW)
  BowVector mBowVec;
  // Frame.cpp:719-726: transform(toDescriptorVector(mDescriptors), mBowVec, mFeatVec, 4) when mBowVec is empty
  void ComputeBoW(const ORBVocabulary& voc);
  // PnPsolver only: mvKeyRays, mvLevelSigma2, and for the map point a candidate's SearchByBoW matched to key point i (vpMapPointMatches[i] >= 0)
  // its GetWorldPos() in mvMapPointPos[i] and isBad() in mvbMapPointBad[i] (empty = none is bad)
  std::vector<cv::Vec3f> mvKeyRays;
  std::vector<float> mvLevelSigma2;
  std::vector<uint8_t> mvbMapPointBad;
};

struct KeyFrameView;
struct MapPointView;

class ORBMatcher {
 public:
  ORBMatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
  static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b);   // ORBMatcher.cpp:951-967 (single pair, host)
  // ORBMatcher.cpp:130-251: windows of radius th*scale[octave] around the projections, octave +-1, best Hamming <= TH_HIGH,
  // rotation-histogram consistency.  With LastFrame.mvMapPointPos + CurrentFrame.mTcw the whole function runs on the device
  // (cms_search_by_projection: projection, windows, greedy, histogram).  Otherwise the projections are read from projInCurrent,
  // distances / arg-min run on the GPU (cms_hamming_best2) and the greedy acceptance is replayed on the host in the reference's
  // order.  Returns the number of matches, fills CurrentFrame.mvpMapPoints.
  int SearchByProjection(FrameView& CurrentFrame, const FrameView& LastFrame, float th, bool bMono);
  // ORBMatcher.cpp:50-128, Tracking.cpp:841: search matches between the frame's key points and the projected map points Frame::isInFrustum marked
  // (mbTrackInView with mTrackProjX / Y, mnTrackScaleLevel, mTrackViewCos).  Points not in view are skipped like the reference does; for the
  // others the device repeats isInFrustum on F.mTcw (the same arithmetic gives the same fields) and runs the greedy search with mfNNratio.
  // Fills F.mvpMapPoints with the matched points' ids, returns the number of matches.
  int SearchByProjection(FrameView& F, std::vector<MapPointView>& vpMapPoints, float th = 3.0f);
  // ORBMatcher.cpp:676-794, Tracking.cpp:428-429: level-0 key points of F1 against F2 inside windows around vbPrevMatched (updated for the matches
  // like the reference), best / second best with mfNNratio, take-over of a key point of F2 by a strictly better match, rotation histogram.
  // vnMatches12[i1] = index in F2 or -1; returns the number of matches.  (cms_search_for_initialization)
  int SearchForInitialization(FrameView& F1, FrameView& F2, std::vector<cv::Point2f>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize = 10);
  // ORBMatcher.cpp:971-1125, LocalMapping.cpp:254: features of pKF1 without a map point against those of pKF2 in the same vocabulary node,
  // epipole distance and epipolar gate with E12 (3x3 CV_32F).  vMatchedPairs in ascending idx1.  (cms_search_for_triangulation)
  int SearchForTriangulation(const KeyFrameView& pKF1, const KeyFrameView& pKF2, const cv::Mat& E12, std::vector<std::pair<size_t, size_t>>& vMatchedPairs);
  // ORBMatcher.cpp:1127-1226: search on the device (cms_fuse_search), then the reference's Replace / AddObservation decisions in list
  // order: fused[i] = key point map point i is fused with (or -1); returns nFused.  mvpMapPoints of pKF is updated for additions.
  int Fuse(KeyFrameView& pKF, const std::vector<MapPointView>& vpMapPoints, const std::vector<uint8_t>& skip, float th, std::vector<int>& fused);
  // ORBMatcher.cpp:409-539, Tracking.cpp:578 / 1030: features of pKF with a map point that is not bad against F's features of the same vocabulary
  // node, best / second best with mfNNratio, a frame feature taken once, rotation histogram.  vpMapPointMatches[i] = id of the map point frame key
  // point i receives, or -1; returns nmatches.  (cms_search_by_bow: F's key points and descriptors go to the device first)
  int SearchByBoW(const KeyFrameView& pKF, FrameView& F, std::vector<long>& vpMapPointMatches);
  // ORBMatcher.cpp:541-674, LoopClosing.cpp:264: features of pKF1 with a map point that is not bad against pKF2's features of the same vocabulary
  // node that hold one too and are not taken yet, best < TH_LOW (strict) and the mfNNratio test, rotation histogram.  vpMatches12[i] = id of pKF2's
  // map point key point i of pKF1 receives, or -1; returns nmatches.  (cms_kfstore_search_by_bow_keyframes: both views go into a small store of the
  // shared context first; the device path only, as everywhere in the mirror)
  int SearchByBoW(const KeyFrameView& pKF1, const KeyFrameView& pKF2, std::vector<long>& vpMatches12);
  // ORBMatcher.cpp:253-378, Tracking.cpp:1101 / :1115 (Relocalization's guided search): the map points of pKF that are not bad and not in
  // sAlreadyFound (ids), in key-point order (:268-276), projected with CurrentFrame.mTcw; windows th * scale[predicted level] over level +-1, key
  // points that hold a map point skipped, best Hamming <= ORBdist, rotation histogram with pKF's key-point angles.  Reads pKF.mvMapPoints for the
  // points' position, distances and descriptor.  Fills CurrentFrame.mvpMapPoints with the matched ids, returns nmatches.
  // (cms_search_by_projection_keyframe: the frame's key points and descriptors go to the device first)
  int SearchByProjection(FrameView& CurrentFrame, const KeyFrameView& pKF, const std::set<long>& sAlreadyFound, float th, int ORBdist);
  // ORBMatcher.cpp:1365-1586, LoopClosing.cpp:322: the map points of each key frame that are not bad and not matched yet (vpMatches12 on entry, and
  // through it the key points of pKF2 that observe a matched point: :1390-1400 on ids) are carried into the other camera by the similarity
  // (s12, R12 3x3, t12 3x1, CV_32F), projected, and matched inside windows th * scale[predicted level] over octaves level - 1 and level, best Hamming
  // <= TH_HIGH; a pair is kept where both directions agree.  Reads pKF.mvMapPoints (position, distances, descriptor) and Tcw of both views.
  // vpMatches12[i1] receives the id of pKF2's map point; returns nFound.  zAsWritten: the depth of the 2 -> 1 projection is component 1, line :1507
  // as the reference has it (the default: the product's contract is the reference's result); false takes component 2.
  // (cms_kfstore_search_by_sim3: both views go into the small store of the shared context first; the device path only)
  int SearchBySim3(const KeyFrameView& pKF1, const KeyFrameView& pKF2, std::vector<long>& vpMatches12, float s12, const cv::Mat& R12, const cv::Mat& t12, float th,
                   bool zAsWritten = true);
  // ORBMatcher.cpp:796-903, LoopClosing.cpp:374: vpPoints that are not bad (MapPointView::mbBad) and not among vpMatched on entry (:806-807, :817) are
  // projected through the decomposed Scw (4x4 or 3x4 CV_32F; pKF.Tcw is not read) and matched inside windows th * scale[predicted level] over octaves
  // level - 1 and level; key points with vpMatched[idx] >= 0 -- on entry or through an earlier point of the call -- are passed over; best Hamming
  // <= TH_LOW.  vpMatched (ids, -1 = NULL, one per key point of pKF) receives the matched points; returns nmatches.
  // (cms_kfstore_search_by_projection_sim3: the view goes into the small store of the shared context first; the device path only)
  int SearchByProjection(const KeyFrameView& pKF, const cv::Mat& Scw, const std::vector<MapPointView>& vpPoints, std::vector<long>& vpMatched, int th);
  // ORBMatcher.cpp:1246-1363, LoopClosing.cpp:586-612: vpPoints that are not bad and not among pKF's map points that are not bad (GetMapPoints, :1256,
  // :1268) are projected through the decomposed Scw and matched as above without the vpMatched test.  In list order (:1345-1359): where the key point
  // holds a map point that is not bad, vpReplacePoint[iMP] receives its id; where it holds a bad one nothing; a free key point receives the point
  // (AddObservation / AddMapPoint: pKF.mvpMapPoints[bestIdx] = the id, which is why pKF is not const here).  vpReplacePoint must have one entry per
  // point; returns nFused.  (cms_kfstore_fuse_search_sim3)
  int Fuse(KeyFrameView& pKF, const cv::Mat& Scw, const std::vector<MapPointView>& vpPoints, float th, std::vector<long>& vpReplacePoint);
  static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 12;

 protected:
  float mfNNratio;
  bool mbCheckOrientation;
};

// What Frame::isInFrustum and ORBMatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) read and write on a MapPoint
// (include/MapPoint.h): position, mean viewing direction, scale-invariance distances, representative descriptor, and the
// mbTrackInView / mTrackProj* / mnTrackScaleLevel / mTrackViewCos fields Tracking uses afterwards.
struct MapPointView {
  long mnId = -1;
  bool mbBad = false;                   // isBad(), where a function reads it from the point (the Scw matchers of loop closing)
  cv::Mat mWorldPos, mNormalVector;     // 3x1 CV_32F
  float mfMinDistance = 0, mfMaxDistance = 0;
  cv::Mat mDescriptor;                  // 1x32 CV_8U
  bool mbTrackInView = false;
  float mTrackProjX = -1, mTrackProjY = -1, mTrackViewCos = 0;
  int mnTrackScaleLevel = -1;
};

// PnPsolver (include/PnPsolver.h, src/PnPsolver.cpp) under the reference's names: the constructor's filtering and order (:83-108), SetRansacParameters
// with the header's defaults, find / iterate returning the 4 x 4 CV_32F pose or an empty cv::Mat, vbInliers expanded through mvKeyPointIndices.
// iterate() makes the call's draws first -- 4 per iteration the loop of :184 may need -- through the replaceable `draw` (default: DUtils::Random::RandomInt,
// DUtils/Random.cpp:47-50), then runs the loop in one cms_pnp_iterate call on the shared context's device (engine DEVICE, the default) or through the
// host build of the same core (engine HOST_CORE: the definition of record, no GPU needed).  When a call ends early the draws behind the accepting
// iteration are discarded: the contract is the reference's loop on the same draws, not the same rand() consumption.
class PnPsolver {
 public:
  enum Engine { DEVICE = 0, HOST_CORE = 1 };
  PnPsolver(const FrameView& F, const std::vector<long>& vpMapPointMatches);
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991);
  cv::Mat find(std::vector<bool>& vbInliers, int& nInliers);
  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);
  std::function<int(int, int)> draw;      // RandomInt(min, max)
  Engine engine = DEVICE;
  // the reference's members, for callers and tests that look at them
  std::vector<cv::Point2f> mvP2D;
  std::vector<cv::Vec3f> mvBearings, mvP3Dw;
  std::vector<float> mvSigma2;
  std::vector<size_t> mvKeyPointIndices;
  int N = 0, mnIterations = 0, mnBestInliers = 0, mRansacMinInliers = 0, mRansacMaxIts = 0, mRansacMinSet = 4;
  float mRansacEpsilon = 0, mRansacTh2 = 5.991f;
  std::vector<uint8_t> mvbBestInliers;
  float mBestTcw[12] = {0};

 private:
  size_t nMatches_ = 0;      // mvpMapPointMatches.size(): the length of vbInliers
};

// What Sim3Solver's constructor (src/Sim3Solver.cpp:41-136) reads of a key frame and of its map points: GetRotation / GetTranslation, mvKeys[i].octave,
// mvLevelSigma2, GetMapPointMatches() (key frame 1 only) and per map point GetWorldPos(), isBad() and GetIndexInKeyFrame(this key frame).
struct Sim3MapPointView {
  cv::Vec3f mWorldPos;
  bool mbBad = false;
  int mnIndexInKeyFrame = -1;
};
struct Sim3KeyFrameView {
  float Rcw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tcw[3] = {0, 0, 0};
  std::vector<int> mvKeyOctaves;               // mvKeys[i].octave
  std::vector<float> mvLevelSigma2;
  std::vector<Sim3MapPointView> mvMapPoints;   // the map points this key frame's side of the matches refers to
  std::vector<int> mvpMapPointMatches;         // per key point: index into mvMapPoints, -1 = none (GetMapPointMatches)
};

// Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cpp) under the reference's names, for LoopClosing::ComputeSim3 (LoopClosing.cpp:270-330): the
// constructor's filtering and order (:66-127; vpMatched12[i1] = index into pKF2.mvMapPoints of the map point matched to key point i1 of pKF1, -1 = none),
// Rcw Xw + tcw per point, mvnMaxError = 9.210 * sigma2, SetRansacParameters with the header's defaults, iterate / find returning the 4 x 4 CV_32F
// mBestT12 or an empty cv::Mat, vbInliers expanded through mvnIndices1 to size mN1, GetEstimatedRotation / Translation / Scale.  iterate() makes the
// call's draws first -- three per iteration, for max(mRansacMaxIts - mnIterations, nIterations) iterations -- through the replaceable `draw`
// (default: DUtils::Random::RandomInt), then runs the loop in one cms_sim3_iterate call on the shared context's device (engine DEVICE, the default) or
// through the host build of the same core (engine HOST_CORE: the definition of record, no GPU needed; an explicit choice, never a fall-back).  The
// contract is the reference's loop on the same draws, not the same rand() consumption.
class Sim3Solver {
 public:
  enum Engine { DEVICE = 0, HOST_CORE = 1 };
  Sim3Solver(const Sim3KeyFrameView& pKF1, const Sim3KeyFrameView& pKF2, const std::vector<int>& vpMatched12, const bool bFixScale = true);
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);
  cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers);
  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);
  cv::Mat GetEstimatedRotation();
  cv::Mat GetEstimatedTranslation();
  float GetEstimatedScale();
  std::function<int(int, int)> draw;      // RandomInt(min, max)
  Engine engine = DEVICE;
  // the reference's members, for callers and tests that look at them
  std::vector<cv::Vec3f> mvX3Dc1, mvX3Dc2;
  std::vector<float> mvnMaxError1, mvnMaxError2;
  std::vector<size_t> mvnIndices1;
  int N = 0, mN1 = 0, mnIterations = 0, mnBestInliers = 0, mRansacMinInliers = 0, mRansacMaxIts = 0;
  double mRansacProb = 0;
  bool mbFixScale = true;
  std::vector<uint8_t> mvbBestInliers;
  float mBestRotation[9] = {0}, mBestTranslation[3] = {0}, mBestScale = 0, mBestT12[12] = {0};
};

// Initializer (include/Initializer.h, src/Initializer.cpp) under the reference's names, for Tracking::MonocularInitialization (Tracking.cpp:409, :443): the
// constructor keeps the reference frame's key points and key rays, InitializeWithRays filters vMatches12 into mvMatches12 (:61-73), makes the
// 8 * mMaxIterations draws through the replaceable `draw` and resolves them into mvSets by swap-and-pop (:92-107), then runs FindEssential and
// ReconstructE in one cms_init_two_view call on the shared context's device (engine DEVICE, the default) or through the host build of the same core
// (engine HOST_CORE: the definition of record, no GPU needed).  The default draw seeds rand() with 0 once per process (DUtils::Random::SeedRandOnce(0))
// and applies DUtils::Random::RandomInt's formula (Random.cpp:38-50).  On false R21 and t21 are empty and vP3D / vbTriangulated are left as they
// were, like the reference; fewer than 8 matches return false (the reference would index an empty vector).
class Initializer {
 public:
  enum Engine { DEVICE = 0, HOST_CORE = 1 };
  Initializer(const FrameView& ReferenceFrame, float sigma = 1.0, int iterations = 200);
  bool InitializeWithRays(const FrameView& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,
                          std::vector<bool>& vbTriangulated);
  std::function<int(int, int)> draw;      // RandomInt(min, max)
  Engine engine = DEVICE;
  // the reference's members, for callers and tests that look at them
  std::vector<cv::KeyPoint> mvKeys1, mvKeys2;
  std::vector<cv::Vec3f> mvKeyRays1, mvKeyRays2;
  typedef std::pair<int, int> Match;
  std::vector<Match> mvMatches12;
  std::vector<bool> mvbMatched1;
  std::vector<std::vector<size_t>> mvSets;
  float mSigma, mSigma2;
  int mMaxIterations;
  // diagnostics of the last attempt (cms_init_job): iteration of the best hypothesis, its score and inliers, nGood / parallax of the four motions, winner
  int mnBestIteration = -1, mnInliers = 0, mnGood[4] = {0, 0, 0, 0}, mnWinner = -1;
  float mfScore = 0, mfParallax[4] = {0, 0, 0, 0};
};

// Tracking::SearchLocalPoints (src/Tracking.cpp:794-846): Frame::isInFrustum(pMP, 0.5) for every local map point, then
// ORBMatcher(0.8).SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th).  Both halves run on the device in one call
// (cms_search_local_points); F.mTcw is the 4x4 CV_32F pose (Frame::SetPose), F.mvpMapPoints gets the id of the matched point.
class Tracking {
 public:
  static int SearchLocalPoints(FrameView& F, std::vector<MapPointView>& vpLocalMapPoints, float th = 1.0f, float nnratio = 0.8f,
                               float viewingCosLimit = 0.5f);
};

// The window Optimizer::LocalBundleAdjustment assembles from pKF's covisibility graph (Optimizer.cpp:194-357), as data.
struct LocalBAWindow {
  struct KF { long mnId; cv::Mat Tcw; bool fixed; std::vector<float> mvInvLevelSigma2; };   // Tcw: 4x4 CV_32F
  struct Obs { int kf; cv::KeyPoint kp; cv::Vec3f ray; };                                   // kf = index into keyframes
  struct MP { long mnId; cv::Mat Xw; std::vector<Obs> observations; };                      // Xw: 3x1 CV_32F
  std::vector<KF> keyframes;
  std::vector<MP> mappoints;
  std::vector<std::pair<int, int>> toErase;   // out: (keyframe index, map point index) observations to erase
};

// The members of Frame that Optimizer::PoseOptimization reads and writes (Frame.h: mTcw, N, mvKeys, mvKeyRays, mvpMapPoints,
// mvbOutlier, mvInvLevelSigma2); a map point is represented by its world position (MapPoint::GetWorldPos()).
struct PoseFrame {
  cv::Mat mTcw;                                 // 4x4 CV_32F, in/out (Frame::SetPose)
  int N = 0;
  std::vector<cv::KeyPoint> mvKeys;
  std::vector<cv::Vec3f> mvKeyRays;
  std::vector<bool> mvbHasMapPoint;             // mvpMapPoints[i] != NULL
  std::vector<cv::Vec3f> mvMapPointPos;         // pMP->GetWorldPos() where mvbHasMapPoint[i]
  std::vector<bool> mvbOutlier;                 // out
  std::vector<float> mvInvLevelSigma2;
};

// What LocalMapping::CreateNewMapPoints, ORBMatcher::SearchForTriangulation and ORBMatcher::Fuse read of a KeyFrame
// (include/KeyFrame.h): key points, descriptors, key rays, the map-point slot per key point (>= 0 = id), pose, mFeatVec
// (DBoW2::FeatureVector: node id -> feature indices, std::map order) and ComputeSceneMedianDepth(2).
struct KeyFrameView {
  long mnId = -1;
  std::vector<cv::KeyPoint> mvKeys;
  cv::Mat mDescriptors;                                  // N x 32 CV_8U
  std::vector<cv::Vec3f> mvKeyRays;
  std::vector<long> mvpMapPoints;                        // -1 = none
  std::vector<uint8_t> mvbMapPointBad;                   // per key point: the map point isBad() (SearchByBoW); empty = none is bad
  cv::Mat Tcw;                                           // 4x4 CV_32F
  std::vector<std::pair<unsigned, std::vector<unsigned>>> mFeatVec;   // ascending node id
  BowVector mBowVec;
  // KeyFrame.cpp:94-103: the same transform when mBowVec or mFeatVec is empty
  void ComputeBoW(const ORBVocabulary& voc);
  float medianDepth = 1.0f;                              // ComputeSceneMedianDepth(2)
  // per key point with mvpMapPoints[i] >= 0: what SearchByProjection(Frame&, KeyFrame*, ...) reads of that map point (GetWorldPos, GetDescriptor,
  // mfMinDistance / mfMaxDistance); empty for the callers that do not need it
  std::vector<MapPointView> mvMapPoints;
};
struct NewMapPoint { int neighbour; int idx1, idx2; cv::Vec3f x3D; };
// KeyFrameDatabase under the reference's names (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cpp) on KeyFrameView handles.  Two engines like the
// vocabulary's: DEVICE (the default) keeps the key frames in a cms_kfstore on the shared context's device with the BowVectors the views carry
// (cms_kfstore_put, cms_kfstore_set_bow, cms_kfdb_add) and answers with cms_kfdb_detect; HOST_CORE is the host build of csrc/cms_kfdb_core.h, the
// definition of record, no GPU needed.  Choose the engine before the first add: each engine answers from the key frames it was given.  The view has no
// covisibility graph, so SetBestCovisibilityKeyFrames hands over what pKF->GetBestCovisibilityKeyFrames(10) returns, and DetectLoopCandidates takes
// pKF->GetConnectedKeyFrames() as an argument.  A vocabulary whose scoring is not L1 throws std::runtime_error, as ORBVocabulary::score does; so does a
// key frame beyond max_keyframes or with more words or features than max_features.
class KeyFrameDatabase {
 public:
  enum Engine { DEVICE = 0, HOST_CORE = 1 };
  explicit KeyFrameDatabase(const ORBVocabulary& voc, int max_keyframes = 256, int max_features = 2048);
  ~KeyFrameDatabase();
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;
  void add(KeyFrameView* pKF);             // :45-51 (pKF->mBowVec must be computed)
  void erase(KeyFrameView* pKF);           // :53-72
  void clear();                            // :74-78
  void SetBestCovisibilityKeyFrames(KeyFrameView* pKF, const std::vector<KeyFrameView*>& best);
  std::vector<KeyFrameView*> DetectRelocalizationCandidates(FrameView* F);                                                    // :204-314
  std::vector<KeyFrameView*> DetectLoopCandidates(KeyFrameView* pKF, float minScore, const std::vector<KeyFrameView*>& connected);   // :81-202
  Engine engine = DEVICE;

 private:
  struct Impl;
  Impl* impl_;
};

// The covisibility bookkeeping under the reference's names on KeyFrameView handles: KeyFrame::UpdateConnections (KeyFrame.cpp:315-404),
// LocalMapping::KeyFrameCulling (LocalMapping.cpp:561-619), Tracking::UpdateLocalKeyFrames' votes and max rule (Tracking.cpp:881-928) and
// Tracking::UpdateLocalPoints (:855-878).  Two engines, an explicit choice and never a fall-back: DEVICE keeps the members in a cms_kfstore on the shared
// context's device and answers with cms_covis_*; HOST_CORE is the host build of csrc/cms_covis_core.h, the definition of record, no GPU needed.
// Build() hands over the map's key frames that are not bad, in the order that then decides ties (the reference's pointer order is the allocator's
// business); a map point is mvpMapPoints[i] >= 0 with mvbMapPointBad[i] == 0, named by its id & 0x3FFFFFFF.  Every method answers from the last Build.
// This is a parity mirror, not the intended usage: the DEVICE engine keeps a private store and puts EVERY member into it again on each Build (key
// points, descriptors, rays and the grid build included).  A host that tracks keeps its key frames resident and sends only what changed
// (cms_kfstore_update_map_points), as the bridge's Hip::BuildCovisibility does.
class Covisibility {
 public:
  enum Engine { DEVICE = 0, HOST_CORE = 1 };
  explicit Covisibility(Engine engine, int max_keyframes = 256, int max_features = 2048);
  ~Covisibility();
  Covisibility(const Covisibility&) = delete;
  Covisibility& operator=(const Covisibility&) = delete;
  void Build(const std::vector<KeyFrameView*>& members);
  // mConnectedKeyFrameWeights (members with weight 0 left out), mvpOrderedConnectedKeyFrames and mvOrderedWeights of pKF; AddConnection on the others,
  // the parent and the spanning tree stay with the caller
  struct Connections { std::map<KeyFrameView*, int> weights; std::vector<KeyFrameView*> ordered; std::vector<int> orderedWeights; };
  Connections UpdateConnections(KeyFrameView* pKF, int th = 15);
  // one KeyFrameCulling call: the candidates are GetVectorCovisibleKeyFrames() minus mnId == 0 in that order, notErase their mbNotErase.  Per
  // candidate nMPs, nRedundantObservations and the verdict; SetBadFlag on the redundant ones stays with the caller
  struct Culled { KeyFrameView* pKF; int nMPs, nRedundantObservations; bool redundant; };
  std::vector<Culled> KeyFrameCulling(const std::vector<KeyFrameView*>& candidates, const std::vector<bool>& notErase, int thObs = 3);
  // the frame's non-NULL, non-bad map points as ids: the key frames with a vote in member order (mvpLocalKeyFrames before the neighbours are added),
  // their votes, and pKFmax (NULL: keyframeCounter is empty)
  std::vector<KeyFrameView*> UpdateLocalKeyFrames(const std::vector<long>& framePoints, KeyFrameView** pKFmax, std::vector<int>* votes = nullptr);
  // mvpLocalMapPoints as ids
  std::vector<long> UpdateLocalPoints(const std::vector<KeyFrameView*>& localKeyFrames);

 private:
  struct Impl;
  Impl* impl_;
};

// The map points' derived members under the reference's names: MapPoint::ComputeDistinctiveDescriptors (MapPoint.cpp:243-308) and
// MapPoint::UpdateNormalAndDepth (:332-373) over the key frames of the last Build, a map point named by its id (the value in mvpMapPoints, below
// max_points).  Two engines, an explicit choice and never a fall-back: DEVICE keeps the members in a cms_kfstore with a cms_covis and a cms_mpstore
// on the shared context's device; HOST_CORE is the host build of csrc/cms_mappoint_core.h, the definition of record, no GPU needed.  Observations are
// taken in the order of Build's list (the reference's std::map<KeyFrame*, size_t> iterates by pointer).  A parity mirror like Covisibility: the
// DEVICE engine puts every member into a private store again on each Build.
class MapPointStore {
 public:
  enum Engine { DEVICE = 0, HOST_CORE = 1 };
  enum { DESCRIPTOR = 1, NORMAL_DEPTH = 2 };
  explicit MapPointStore(Engine engine, int max_keyframes = 256, int max_features = 2048, int max_points = 65536);
  ~MapPointStore();
  MapPointStore(const MapPointStore&) = delete;
  MapPointStore& operator=(const MapPointStore&) = delete;
  void Build(const std::vector<KeyFrameView*>& members);
  // SetWorldPos and mpRefKF of the named points (pRefKF: any key frame of the last Build)
  struct MapPointView { long id; float pos[3]; KeyFrameView* pRefKF; };
  void SetMapPoints(const std::vector<MapPointView>& points);
  void EraseMapPoints(const std::vector<long>& ids);
  // per id: 0 done, 1 no observation among the members (the reference's early return), 2 pRefKF does not observe the point; 1 and 2 leave the row as it was
  std::vector<unsigned char> Refresh(const std::vector<long>& ids, int what = DESCRIPTOR | NORMAL_DEPTH);
  // mDescriptor, mNormalVector, mfMinDistance, mfMaxDistance and the observation the descriptor came from (NULL, -1: none)
  struct Row { float pos[3], normal[3], minDistance, maxDistance; unsigned char descriptor[32]; KeyFrameView* pBestKF; int bestIdx; };
  std::vector<Row> Fetch(const std::vector<long>& ids);
  // The window Optimizer::LocalBundleAdjustment collects (Optimizer.cpp:194-357) from the key frames of the last Build and the points that were set:
  // lLocalKeyFrames is pKF followed by its GetVectorCovisibleKeyFrames(), the key frame of mnId 0 is looked up among the members.  DEVICE: one
  // cms_covis_local_ba_windows call on the private store (key points, rays and poses as Build put them); HOST_CORE: the host build of
  // csrc/cms_ba_window_core.h over the same views.  The arrays are cms_ba_create's arguments; keyframes[k] is the view behind pose k, and
  // (keyframes[e_pose[e]], e_feat[e]) names the observation of edge e.  This class, not Covisibility, carries the method: it is the mirror that holds
  // an index and a table of one store.
  struct BAWindow {
    std::vector<KeyFrameView*> keyframes;
    int nLocal = 0;
    std::vector<long> point_id;
    std::vector<double> poses, points, e_obs, e_invsig2;      // 7 per pose (t, q), 3 per point, 2 per edge, 1 per edge
    std::vector<uint8_t> fixed;
    std::vector<int> e_pose, e_point, e_feat;
    std::vector<int8_t> e_face;
    std::vector<std::pair<KeyFrameView*, int>> toErase;      // out of Optimizer::LocalBundleAdjustment: (key frame, feature) observations to erase
  };
  BAWindow LocalBAWindow(const std::vector<KeyFrameView*>& lLocalKeyFrames);
  // SetPose / SetWorldPos of an optimised window (Optimizer.cpp:432-450): the local key frames' Tcw and the points' positions through float
  // (Converter.cpp:53-104), into the views and into the engine's store (cms_kfstore_update_poses, cms_mpstore_set)
  void WriteBack(const BAWindow& window);

  // ---- the points' counters and what reads them (csrc/cms_mpstats_core.h; DEVICE: cms_mpstore_set_stats / count / culling,
  // cms_covis_tracked_map_points, cms_kfstore_scene_median_depth; HOST_CORE: hm_mpstats_* on the same table)
  // mnFirstKFid, mnVisible and mnFound of points that were set (a negative nVisible / nFound leaves the counter; nFirstKFid < -1 leaves it)
  struct MapPointStats { long id; int nFirstKFid, nVisible, nFound; };
  void SetStatistics(const std::vector<MapPointStats>& stats);
  std::vector<MapPointStats> FetchStatistics(const std::vector<long>& ids);
  // The statistics loop of Tracking::TrackLocalMap and SearchLocalPoints for one frame: IncreaseVisible() for the local points with inView[i] != 0
  // (Tracking.cpp:808, :829), IncreaseFound() for the frame's points (-1: none) with outlier[i] == 0 (:698).  Either list may be empty
  void UpdateTrackStatistics(const std::vector<long>& localIds, const std::vector<unsigned char>& inView, const std::vector<long>& frameIds,
                             const std::vector<unsigned char>& outlier);
  // LocalMapping::MapPointCulling (LocalMapping.cpp:175-206) on mlpRecentAddedMapPoints as ids: one culling call with apply, then the list handling
  // of :184-205 (a point that is bad, became bad or is three key frames old leaves the list).  SetBadFlag reaches the engine's store and the views
  // of the last Build (mvpMapPoints -> -1).  Returns the verdicts in the list's order before the call
  std::vector<unsigned char> MapPointCulling(std::list<long>& recentIds, int currentKFid, int thObs = 2);
  // KeyFrame::TrackedMapPoints(minObs) (KeyFrame.cpp:276-301) of a key frame of the last Build, on the rows as they were then
  int TrackedMapPoints(KeyFrameView* pKF, int minObs);
  // KeyFrame::ComputeSceneMedianDepth(q) (KeyFrame.cpp:1064-1094) from the key frame's current row in the store and the points that were set;
  // -1 when it sees none
  float ComputeSceneMedianDepth(KeyFrameView* pKF, int q = 2);

 private:
  struct Impl;
  Impl* impl_;
};

class LocalMapping {
 public:
  // LocalMapping.cpp:209-386 with the covisible neighbours already collected (GetBestCovisibilityKeyFrames(20)): returns the points
  // the reference would create, in creation order; the MapPoint bookkeeping (:359-381) stays with the caller.
  static std::vector<NewMapPoint> CreateNewMapPoints(const KeyFrameView& current, const std::vector<const KeyFrameView*>& vpNeighKFs);
};

// What Optimizer::OptimizeSim3 (src/Optimizer.cpp:888-1091) reads of a key frame beyond what Sim3Solver does: mvKeys[i].pt and mvInvLevelSigma2.
struct Sim3OptKeyFrameView : Sim3KeyFrameView {
  std::vector<cv::Point2f> mvKeyPts;           // mvKeys[i].pt, cubemap image coordinates
  std::vector<float> mvInvLevelSigma2;
};
// g2oS12.  In: R (row major) | t | s, what LoopClosing.cpp:324 hands g2o::Sim3(R, t, s).  Out: q (x y z w) | t | s, the optimised estimate; R is left alone.
struct Sim3Value {
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1;
  double q[4] = {0, 0, 0, 1};
};
// The graph of :939-1028 as the arrays of one cms_sim3_opt_job; vnIndexEdge[k] = the key point of key frame 1 (entry of vpMatches1) behind pair k
struct Sim3OptGraph {
  std::vector<float> x3dc1, x3dc2, kp1, kp2, invSigma2_1, invSigma2_2;
  std::vector<size_t> vnIndexEdge;
};

// What Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:623-886) reads and writes of the map.  Key frames and map points are named by their index
// in the map's vectors (the order of GetAllKeyFrames / GetAllMapPoints); -1 = none.  The reference's containers are ordered by pointer value, which
// is the allocator's business; the mirror's LoopConnections, loop edges and pose maps iterate in ascending index -- the order of addEdge, and with it
// the order of the sums, is the caller's to choose there too.
struct EssGraphKeyFrameView {
  long unsigned int mnId = 0;
  bool mbBad = false;
  float Tcw[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};      // [R | t] row major; SetPose writes it (:833-852)
  int mpParent = -1;
  std::set<int> mspChildrens, mspLoopEdges;
  std::vector<int> mvpOrderedConnectedKeyFrames, mvOrderedWeights;      // covisibles by descending weight (GetCovisiblesByWeight, GetWeight)
};
struct EssGraphMapPointView {
  bool mbBad = false;
  float mWorldPos[3] = {0, 0, 0};                                  // SetWorldPos writes it (:854-885)
  int mpRefKF = -1;
  long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
};
struct EssentialGraphMap {
  std::vector<EssGraphKeyFrameView> mvpKeyFrames;
  std::vector<EssGraphMapPointView> mvpMapPoints;
};
struct Sim3Pose { double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1; };      // g2o::Sim3: q (x y z w) | t | s
typedef std::map<int, Sim3Pose> KeyFrameAndPose;                                 // LoopClosing::KeyFrameAndPose by key-frame index
// The graph of :650-825 as the arrays of one cms_ess_graph_job: vertex v is key frame vertexKF[v] (the key frames that are not bad, in mnId order)
struct EssGraph {
  std::vector<int> vertexKF, edges;      // edges: v0, v1, kind
  std::vector<double> Scw, Snc;          // 8 per vertex
  int fixed = -1;
};

// What Optimizer::GlobalBundleAdjustemnt / BundleAdjustment (src/Optimizer.cpp:453-621) reads and writes of the map.  Key frames and map points are
// named by their index in the map's vectors (the order of GetAllKeyFrames / GetAllMapPoints).  An observation names a key frame by its index in
// mvpKeyFrames; the first nListedKeyFrames of them are the call's vpKFs, any further ones stand for key frames the map received after the snapshot (the
// reference skips their observations: mnId > maxKFid, :520).  The reference walks a point's observations in the order of a std::map keyed by pointer,
// which is the allocator's business; the mirror walks them as the caller lists them.
struct GlobalBAKeyFrameView {
  long unsigned int mnId = 0;
  bool mbBad = false;
  cv::Mat Tcw;                                  // 4x4 CV_32F; SetPose writes it when nLoopKF == 0 (:586)
  std::vector<cv::KeyPoint> mvKeys;
  std::vector<cv::Vec3f> mvKeyRays;
  std::vector<float> mvInvLevelSigma2;
  cv::Mat mTcwGBA;                              // 4x4 CV_32F, created and written when nLoopKF != 0 (:590-592)
  long unsigned int mnBAGlobalForKF = 0;
};
struct GlobalBAMapPointView {
  long unsigned int mnId = 0;
  bool mbBad = false;
  cv::Mat Xw;                                   // 3x1 CV_32F; SetWorldPos writes it when nLoopKF == 0 (:610)
  std::vector<std::pair<int, int>> observations;      // (key-frame index, key-point index)
  cv::Mat mPosGBA;                              // 3x1 CV_32F, created and written when nLoopKF != 0 (:615-617)
  long unsigned int mnBAGlobalForKF = 0;
};
struct GlobalBAMap {
  std::vector<GlobalBAKeyFrameView> mvpKeyFrames;
  std::vector<GlobalBAMapPointView> mvpMapPoints;
  int nListedKeyFrames = -1;                    // -1: all of mvpKeyFrames
};
// The graph of :480-568 as the arrays of cms_ba_create: pose k is key frame vertexKF[k] (the listed key frames that are not bad, in list order), point p
// is map point vertexMP[p] (not bad and left with at least one edge, in list order); edges per point in list order, per observation in the point's order
struct GlobalBAGraph {
  std::vector<int> vertexKF, vertexMP;
  std::vector<double> poses, points, e_obs, e_invsig2;      // 7 per pose (t, q), 3 per point, 2 per edge, 1 per edge
  std::vector<uint8_t> fixed;                                // mnId == 0
  std::vector<int> e_pose, e_point;
  std::vector<int8_t> e_face;
  std::vector<uint8_t> vbNotIncludedMP;                      // per map point of the map: bad points are never looked at (0), points without an edge are 1
};

class Optimizer {
 public:
  enum Engine { DEVICE = 0, HOST_CORE = 1 };
  // Optimizer.cpp:453-621, spelled as the reference spells it.  CollectGlobalBA does the pointer work of :480-568: bad key frames and bad map points are
  // left out, fixed = mnId == 0, observations from a bad key frame or from one with mnId > maxKFid are skipped (so are those from a key frame that has no
  // vertex although its mnId is below maxKFid, where the reference would hand g2o a null vertex), rays with z < cosFovTh are skipped, face and in-face
  // measurement come from the key point, invSigma2 is that of the octave, a map point left with no edge is marked not included and never written.  The
  // optimisation is one cms_ba_optimize_global call -- optimize(nIterations), Huber(sqrt(5.99)) if bRobust -- on the shared context's device.  Write-back
  // as :577-619: nLoopKF == 0 into Tcw / Xw through float, otherwise into mTcwGBA / mPosGBA with mnBAGlobalForKF = nLoopKF.  UpdateNormalAndDepth (:611)
  // stays the caller's.
  static void GlobalBundleAdjustemnt(GlobalBAMap& pMap, int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true);
  static GlobalBAGraph CollectGlobalBA(const GlobalBAMap& pMap);
  // Optimizer.cpp:623-886.  CollectEssentialGraph does the pointer work of :650-825: one vertex per key frame that is not bad, in mnId order, with vScw
  // = the CorrectedSim3 value or Sim3(Rcw, tcw, 1); the loop-connection edges under the minFeat = 100 rule with the (pCurKF, pLoopKF) exemption and
  // sInsertedEdges; per key frame the spanning-tree edge, the loop edges to lower mnId and the covisibility edges of weight >= minFeat that are neither
  // parent, child nor loop edge, not bad, of lower mnId and not in sInsertedEdges, measured from NonCorrectedSim3 where present.  An edge to a key
  // frame without a vertex (bad) is left out, where the reference would hand g2o a null vertex.  The optimisation is one
  // cms_essential_graph_optimize call on the shared context's device (engine DEVICE, the default) or the host build of the same core (HOST_CORE: the
  // definition of record, no GPU needed; an explicit choice, never a fall-back).  Poses (:833-852) and map points (:854-885, through
  // cms_sim3_correct_points) are written back; UpdateNormalAndDepth stays the caller's.
  static void OptimizeEssentialGraph(EssentialGraphMap& pMap, int pLoopKF, int pCurKF, const KeyFrameAndPose& NonCorrectedSim3, const KeyFrameAndPose& CorrectedSim3,
                                     const std::map<int, std::set<int>>& LoopConnections, const bool& bFixScale, Engine engine = DEVICE);
  static EssGraph CollectEssentialGraph(const EssentialGraphMap& pMap, int pLoopKF, int pCurKF, const KeyFrameAndPose& NonCorrectedSim3,
                                        const KeyFrameAndPose& CorrectedSim3, const std::map<int, std::set<int>>& LoopConnections);
  // Optimizer.cpp:888-1091.  vpMatches1[i] = index into pKF2.mvMapPoints of the map point matched to key point i of pKF1, -1 = NULL; entries the
  // reference nulls (:1046, :1080) become -1.  The pointer work of :941-978 is CollectSim3Graph: !pMP1 || !pMP2, isBad, GetIndexInKeyFrame(pKF2) < 0,
  // P3D1c / P3D2c = Rcw Xw + tcw by the gemm rule of Sim3Solver's constructor, mvKeys[i].pt / mvKeys[i2].pt, mvInvLevelSigma2[octave].  The rest is
  // one cms_sim3_optimize call on the shared context's device (engine DEVICE, the default) or the host build of the same core (engine HOST_CORE: the
  // definition of record, no GPU needed; an explicit choice, never a fall-back).  jacobian: CMS_SIM3_OPT_AS_WRITTEN (the reference's numeric
  // Jacobian) or CMS_SIM3_OPT_ANALYTIC.  Returns nIn; 0 with g2oS12's q | t | s = the start when fewer than 10 pairs survive the first round.
  static int OptimizeSim3(const Sim3OptKeyFrameView& pKF1, const Sim3OptKeyFrameView& pKF2, std::vector<int>& vpMatches1, Sim3Value& g2oS12, const float th2,
                          const bool bFixScale, Engine engine = DEVICE, int jacobian = 0);
  static Sim3OptGraph CollectSim3Graph(const Sim3OptKeyFrameView& pKF1, const Sim3OptKeyFrameView& pKF2, const std::vector<int>& vpMatches1);

  // Optimizer.cpp:48-190: edges collected exactly like :80-127 (rays with z < cosFovTh skipped, face + in-face measurement of
  // the key point, invSigma2 of its octave, map point through float), the four optimisation rounds run in one GPU kernel
  // (cms_pose_optimize), the pose is written back through float (Converter::toCvMat).  Returns nInitialCorrespondences - nBad.
  static int PoseOptimization(PoseFrame* pFrame);

  // Optimizer.cpp:192-451 with the graph already collected: builds the edge list exactly like :246-357 (fixed = mnId==0 or
  // fixed KF, rays with z < cosFovTh skipped, face + in-face measurement from the key point, invSigma2 of the octave),
  // runs optimize(5) / classify / optimize(10) on the GPU, writes poses and points back through float (Converter.cpp:53-104)
  // and lists the observations to erase.  *pbStopFlag is polled like g2o's forceStopFlag.
  static void LocalBundleAdjustment(LocalBAWindow* window, bool* pbStopFlag);
  // ... with the window assembled from resident data (MapPointStore::LocalBAWindow): cms_ba_run on its arrays as they lie, the outlier edges into
  // window->toErase (:399-412), then MapPointStore::WriteBack.  Nothing is walked on the host.
  static void LocalBundleAdjustment(MapPointStore& mps, MapPointStore::BAWindow* window, bool* pbStopFlag);
};

}  // namespace CubemapSLAM
#endif
