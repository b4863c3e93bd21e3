// CubemapHipBridge.cpp -- see CubemapHipBridge.h.  Compiled inside the reference's tree (OpenCV, Eigen, g2o types); every function gathers
// what the reference function reads into flat arrays, makes ONE call into libcubemapslam_hip.so and writes the result back through the
// reference's own setters, in the reference's order.  Not built in this repository (integration/README.md; syntax-checked by tests/test_integration_syntax.py); the same logic over plain
// structs is cubemapslam_amd/host/cubemap_hot_path.cpp, which is built and tested here.
#include "CubemapHipBridge.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <map>
#include <set>
#include <mutex>
#include <stdexcept>
#include <unistd.h>

#include "CamModelGeneral.h"
#include "Converter.h"
#include "Frame.h"
#include "KeyFrame.h"
#include "Map.h"
#include "MapPoint.h"
#include "ORBMatcher.h"
#include "ThirdParty/DBoW2/DUtils/Random.h"

namespace Hip {
namespace {
double g_fov_deg = 190.0;
int g_device = 0;

void check(int rc, const char* what) {
  if (rc < 0) throw std::runtime_error(std::string(what) + ": " + cms_last_error());
}
void pose7(const cv::Mat& Tcw, double* p) {                       // Converter::toSE3Quat (Converter.cpp:41-51): t then unit quaternion
  const g2o::SE3Quat T = Converter::toSE3Quat(Tcw);
  const Eigen::Vector3d t = T.translation();
  const Eigen::Quaterniond q = T.rotation();
  p[0] = t[0]; p[1] = t[1]; p[2] = t[2]; p[3] = q.x(); p[4] = q.y(); p[5] = q.z(); p[6] = q.w();
}
cv::Mat toMat(const double* p) {                                   // Converter::toCvMat(SE3Quat) (Converter.cpp:53-104): through float
  return Converter::toCvMat(g2o::SE3Quat(Eigen::Quaterniond(p[6], p[3], p[4], p[5]), Eigen::Vector3d(p[0], p[1], p[2])));
}
void kps_to_abi(const std::vector<cv::KeyPoint>& in, std::vector<cms_keypoint>& out) {
  out.resize(in.size());
  for (size_t i = 0; i < in.size(); ++i) out[i] = {in[i].pt.x, in[i].pt.y, in[i].size, in[i].angle, in[i].response, in[i].octave};
}
}  // namespace

void Configure(double camFovDeg, int device) { g_fov_deg = camFovDeg; g_device = device; }   // System::System, next to SetCosFovTh (System.cpp:86-89)

cms_ctx* CreateContext(const cms_orb_params& orb) {
  CamModelGeneral* cam = CamModelGeneral::GetCamera();
  cms_camera c;
  std::memset(&c, 0, sizeof(c));
  c.c = cam->Get_c(); c.d = cam->Get_d(); c.e = cam->Get_e(); c.u0 = cam->Get_u0(); c.v0 = cam->Get_v0();
  const cv::Mat_<double> invP = cam->Get_invP(), P = cam->Get_P();
  for (int i = 0; i < 12 && i < invP.rows; ++i) c.invpol[i] = invP(i, 0);          // zero padded to 12 (System.cpp:70-72)
  for (int i = 0; i < 5 && i < P.rows; ++i) c.pol[i] = P(i, 0);
  c.Iw = cam->GetFisheyeWidth(); c.Ih = cam->GetFisheyeHeight(); c.face = cam->GetCubeFaceWidth(); c.fov_deg = g_fov_deg;
  cms_ctx* ctx = nullptr;
  check(cms_ctx_create(&ctx, g_device, &c, &orb, 1), "cms_ctx_create");
  check(cms_set_distance_bounds_mode(ctx, 1), "cms_set_distance_bounds_mode");     // map points' bounds come from MapPoint's public getters
  // Which 8-bit GaussianBlur (ORBExtractor.cpp:907-908)?  The reference links OpenCV 2.4.11 / 3.2 (README.md:59); on x86 those run the SSE2 column
  // functor (float sums, ties to even) -- definition 1.  A build of the reference on a machine without SSE2 (or against an OpenCV built with
  // -DENABLE_SSE2=OFF) runs the integer column pass: define CUBEMAP_HIP_INTEGER_GAUSSIAN for that one (definition 0, the library's own default).
#ifdef CUBEMAP_HIP_INTEGER_GAUSSIAN
  check(cms_set_gaussian_mode(ctx, 0), "cms_set_gaussian_mode");
#else
  check(cms_set_gaussian_mode(ctx, 1), "cms_set_gaussian_mode");
#endif
  return ctx;
}

void CvtFisheyeToCubeMap(cms_ctx* ctx, cv::Mat& cubemapImg, const cv::Mat& fisheyeImg) {
  check(cms_remap(ctx, fisheyeImg.data, (int)fisheyeImg.step, cubemapImg.data, (int)cubemapImg.step), "cms_remap");   // corner blocks untouched
}

void FrameGrid(cms_ctx* ctx) { check(cms_area_grid(ctx, 1), "cms_area_grid"); }

int SearchForInitialization(cms_ctx* ctx, Frame& F1, Frame& F2, std::vector<cv::Point2f>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize,
                            float nnratio, bool checkOrientation) {
  std::vector<cms_keypoint> k1;
  kps_to_abi(F1.mvKeys, k1);
  vnMatches12.assign(F1.mvKeys.size(), -1);
  int n = 0;
  // cv::Point2f is two floats: vbPrevMatched is the n1 x 2 float array the entry updates in place (ORBMatcher.cpp:786-789)
  check(cms_search_for_initialization(ctx, 0, (int)k1.size(), k1.data(), F1.mDescriptors.data, reinterpret_cast<float*>(vbPrevMatched.data()), windowSize, nnratio,
                                      checkOrientation ? 1 : 0, vnMatches12.data(), &n), "cms_search_for_initialization");
  (void)F2;                                                         // F2 is the frame ctx extracted last: already on the device
  return n;
}

int SearchByProjection(cms_ctx* ctx, Frame& CurrentFrame, const Frame& LastFrame, float th, bool checkOrientation) {
  const int nl = LastFrame.N;
  std::vector<uint8_t> valid(nl, 0), desc((size_t)nl * 32, 0);
  std::vector<float> Xw((size_t)nl * 3, 0.f), angle(nl);
  std::vector<int> octave(nl);
  for (int i = 0; i < nl; ++i) {
    MapPoint* pMP = LastFrame.mvpMapPoints[i];
    octave[i] = LastFrame.mvKeys[i].octave; angle[i] = LastFrame.mvKeys[i].angle;
    if (!pMP || LastFrame.mvbOutlier[i]) continue;                 // ORBMatcher.cpp:153-157
    valid[i] = 1;
    const cv::Mat x = pMP->GetWorldPos();
    for (int k = 0; k < 3; ++k) Xw[3 * i + k] = x.at<float>(k);
    const cv::Mat d = pMP->GetDescriptor();
    std::memcpy(&desc[(size_t)i * 32], d.data, 32);
  }
  float pose12[12];
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) pose12[3 * r + c] = CurrentFrame.mTcw.at<float>(r, c); pose12[9 + r] = CurrentFrame.mTcw.at<float>(r, 3); }
  const int N = CurrentFrame.N;
  std::vector<int> kp_mp(N), match(nl, -1);
  for (int i = 0; i < N; ++i) {                                    // a key point that already holds a map point WITH observations is skipped (:191-193)
    MapPoint* p = CurrentFrame.mvpMapPoints[i];
    kp_mp[i] = (p && p->Observations() > 0) ? (1 << 30) : -1;
  }
  int n = 0;
  check(cms_search_by_projection(ctx, 0, pose12, nl, valid.data(), Xw.data(), octave.data(), angle.data(), desc.data(), th, checkOrientation ? 1 : 0,
                                 ORBMatcher::TH_HIGH, N, kp_mp.data(), match.data(), &n), "cms_search_by_projection");
  for (int i = 0; i < nl; ++i) if (match[i] >= 0) CurrentFrame.mvpMapPoints[match[i]] = LastFrame.mvpMapPoints[i];
  return n;
}

int SearchLocalPoints(cms_ctx* ctx, Frame& F, const std::vector<MapPoint*>& vpMapPoints, float th) {
  // the caller (Tracking::SearchLocalPoints, Tracking.cpp:797-822) has removed the points already matched in the frame and the bad ones
  const int n = (int)vpMapPoints.size();
  std::vector<float> pos((size_t)n * 3), nrm((size_t)n * 3), dmin(n), dmax(n), px(n), py(n), vc(n);
  std::vector<uint8_t> desc((size_t)n * 32), inview(n);
  std::vector<int> level(n), match(n);
  for (int i = 0; i < n; ++i) {
    MapPoint* p = vpMapPoints[i];
    const cv::Mat x = p->GetWorldPos(), nn = p->GetNormal();
    for (int k = 0; k < 3; ++k) { pos[3 * i + k] = x.at<float>(k); nrm[3 * i + k] = nn.at<float>(k); }
    dmin[i] = p->GetMinDistanceInvariance();                       // the PUBLIC getters (MapPoint.cpp:375-385: 0.8f / 1.2f applied); the context was put
    dmax[i] = p->GetMaxDistanceInvariance();                       // into cms_set_distance_bounds_mode(ctx, 1) by the bridge's set-up: MapPoint.h stays untouched
    const cv::Mat d = p->GetDescriptor();
    std::memcpy(&desc[(size_t)i * 32], d.data, 32);
  }
  float pose15[15];
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) pose15[3 * r + c] = F.mTcw.at<float>(r, c); pose15[9 + r] = F.mTcw.at<float>(r, 3); }
  const cv::Mat Ow = F.GetCameraCenter();
  for (int k = 0; k < 3; ++k) pose15[12 + k] = Ow.at<float>(k);
  std::vector<int> kp_mp(F.N);
  for (int i = 0; i < F.N; ++i) { MapPoint* p = F.mvpMapPoints[i]; kp_mp[i] = (p && p->Observations() > 0) ? (1 << 30) : -1; }   // ORBMatcher.cpp:91-95
  int nm = 0;
  check(cms_search_local_points(ctx, 0, pose15, n, pos.data(), nrm.data(), dmin.data(), dmax.data(), desc.data(), 0.5f, th, 0.8f, ORBMatcher::TH_HIGH, F.N,
                                kp_mp.data(), inview.data(), px.data(), py.data(), level.data(), vc.data(), match.data(), &nm, nullptr), "cms_search_local_points");
  for (int i = 0; i < n; ++i) {                                    // what Frame::isInFrustum leaves on the MapPoint (Frame.cpp:199-248) ...
    MapPoint* p = vpMapPoints[i];
    p->mbTrackInView = inview[i] != 0;
    if (!inview[i]) continue;
    p->mTrackProjX = px[i]; p->mTrackProjY = py[i]; p->mnTrackScaleLevel = level[i]; p->mTrackViewCos = vc[i];
    p->IncreaseVisible();                                          // Tracking.cpp:829
    if (match[i] >= 0) F.mvpMapPoints[match[i]] = p;               // ... and what the matcher leaves in the frame (ORBMatcher.cpp:121)
  }
  return nm;
}

int PoseOptimization(Frame* pFrame) {
  CamModelGeneral* cam = CamModelGeneral::GetCamera();
  const int N = pFrame->N;
  std::vector<double> Xw, obs, inv;
  std::vector<int8_t> face;
  std::vector<int> index;
  {
    std::unique_lock<std::mutex> lock(MapPoint::mGlobalMutex);
    for (int i = 0; i < N; ++i) {
      if (pFrame->mvKeyRays[i](2) < cam->GetCosFovTh()) continue;  // Optimizer.cpp:84-86
      MapPoint* pMP = pFrame->mvpMapPoints[i];
      if (!pMP) continue;
      pFrame->mvbOutlier[i] = false;
      const cv::KeyPoint& kp = pFrame->mvKeys[i];
      double u, v;
      cam->GetPosInFace(u, v, (double)kp.pt.x, (double)kp.pt.y);
      obs.push_back(u); obs.push_back(v);
      face.push_back((int8_t)cam->FaceInCubemap(kp.pt));
      inv.push_back(pFrame->mvInvLevelSigma2[kp.octave]);
      const cv::Mat x = pMP->GetWorldPos();
      for (int k = 0; k < 3; ++k) Xw.push_back(x.at<float>(k));
      index.push_back(i);
    }
  }
  const int n = (int)index.size();
  if (n < 3) return 0;                                             // Optimizer.cpp:133-134
  double p[7];
  pose7(pFrame->mTcw, p);
  std::vector<uint8_t> outlier(n, 0);
  int n_in = 0;
  check(cms_pose_optimize(g_device, n, Xw.data(), obs.data(), inv.data(), face.data(), cam->Get_fx(), cam->Get_fy(), cam->Get_cx(), cam->Get_cy(), p, outlier.data(),
                          &n_in, nullptr), "cms_pose_optimize");
  for (int j = 0; j < n; ++j) pFrame->mvbOutlier[index[j]] = outlier[j] != 0;
  pFrame->SetPose(toMat(p));                                       // Optimizer.cpp:184-187
  return n_in;                                                     // nInitialCorrespondences - nBad
}

void SetDeterministic(bool on) { cms_ba_set_deterministic(on ? 64 : 0); }      // (64 workgroups per window: this bridge optimises one window per call)
bool GetDeterministic() { return cms_ba_get_deterministic() != 0; }

void LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap) {
  CamModelGeneral* cam = CamModelGeneral::GetCamera();
  // ---- the window: local key frames, the map points they see, fixed key frames that see those (Optimizer.cpp:194-245)
  std::vector<KeyFrame*> kfs;                                      // local first, then fixed
  std::map<KeyFrame*, int> kf_index;
  auto add_kf = [&](KeyFrame* k) { kf_index[k] = (int)kfs.size(); kfs.push_back(k); };
  add_kf(pKF);
  pKF->mnBALocalForKF = pKF->mnId;
  for (KeyFrame* k : pKF->GetVectorCovisibleKeyFrames()) { k->mnBALocalForKF = pKF->mnId; if (!k->isBad()) add_kf(k); }
  const int n_local = (int)kfs.size();
  std::vector<MapPoint*> mps;
  for (int j = 0; j < n_local; ++j)
    for (MapPoint* p : kfs[j]->GetMapPointMatches())
      if (p && !p->isBad() && p->mnBALocalForKF != pKF->mnId) { mps.push_back(p); p->mnBALocalForKF = pKF->mnId; }
  for (MapPoint* p : mps)
    for (const auto& ob : p->GetObservations()) {
      KeyFrame* k = ob.first;
      if (k->mnBALocalForKF != pKF->mnId && k->mnBAFixedForKF != pKF->mnId) { k->mnBAFixedForKF = pKF->mnId; if (!k->isBad()) add_kf(k); }
    }
  // ---- flat problem (what :262-357 hands g2o): poses, fixed flags (fixed cameras and key frame 0), points, one edge per observation
  const int K = (int)kfs.size(), P = (int)mps.size();
  std::vector<double> poses((size_t)K * 7), points((size_t)P * 3), e_obs, e_inv;
  std::vector<uint8_t> fixed(K);
  std::vector<int> e_pose, e_point;
  std::vector<int8_t> e_face;
  for (int j = 0; j < K; ++j) { pose7(kfs[j]->GetPose(), &poses[(size_t)j * 7]); fixed[j] = (j >= n_local || kfs[j]->mnId == 0) ? 1 : 0; }
  for (int i = 0; i < P; ++i) {
    const cv::Mat x = mps[i]->GetWorldPos();
    for (int k = 0; k < 3; ++k) points[(size_t)i * 3 + k] = x.at<float>(k);
    for (const auto& ob : mps[i]->GetObservations()) {
      KeyFrame* k = ob.first;
      if (k->isBad()) continue;
      if (k->mvKeyRays[ob.second](2) < cam->GetCosFovTh()) continue;            // :323-325
      const cv::KeyPoint& kp = k->mvKeys[ob.second];
      double u, v;
      cam->GetPosInFace(u, v, (double)kp.pt.x, (double)kp.pt.y);
      e_pose.push_back(kf_index[k]); e_point.push_back(i); e_obs.push_back(u); e_obs.push_back(v);
      e_inv.push_back(k->mvInvLevelSigma2[kp.octave]); e_face.push_back((int8_t)cam->FaceInCubemap(kp.pt));
    }
  }
  const int E = (int)e_pose.size();
  if (E == 0) return;
  std::vector<uint8_t> erase(E, 0);
  cms_ba_stats st;
  const int rc = cms_ba_run(g_device, K, poses.data(), fixed.data(), P, points.data(), E, e_pose.data(), e_point.data(), e_obs.data(), e_inv.data(), e_face.data(),
                            cam->Get_fx(), cam->Get_fy(), cam->Get_cx(), cam->Get_cy(), 5, 10, reinterpret_cast<const volatile uint8_t*>(pbStopFlag), erase.data(), &st);
  check(rc, "cms_ba_run");
  if (rc == 1) return;                                              // stop requested before the optimisation started (:359-361)
  // ---- write-back under the map mutex (:419-450)
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  for (int e = 0; e < E; ++e) {
    if (!erase[e]) continue;
    MapPoint* p = mps[e_point[e]];
    if (p->isBad()) continue;
    KeyFrame* k = kfs[e_pose[e]];
    k->EraseMapPointMatch(p);
    p->EraseObservation(k);
  }
  for (int j = 0; j < n_local; ++j) kfs[j]->SetPose(toMat(&poses[(size_t)j * 7]));
  for (int i = 0; i < P; ++i) {
    cv::Mat x(3, 1, CV_32F);
    for (int k = 0; k < 3; ++k) x.at<float>(k) = (float)points[(size_t)i * 3 + k];
    mps[i]->SetWorldPos(x);
    mps[i]->UpdateNormalAndDepth();
  }
}

void GlobalBundleAdjustemnt(Map* pMap, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust) {
  CamModelGeneral* cam = CamModelGeneral::GetCamera();
  const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();    // Optimizer.cpp:455-456
  const std::vector<MapPoint*> vpMP = pMap->GetAllMapPoints();
  // ---- flat problem (what :480-568 hands g2o): one pose per key frame that is not bad, fixed = mnId == 0; one point per map point that is not bad and keeps an edge
  std::vector<KeyFrame*> kfs;
  std::map<KeyFrame*, int> kf_index;
  std::vector<double> poses, points, e_obs, e_inv;
  std::vector<uint8_t> fixed;
  std::vector<int> e_pose, e_point;
  std::vector<int8_t> e_face;
  long unsigned int maxKFid = 0;
  for (KeyFrame* k : vpKFs) {
    if (k->isBad()) continue;
    double p[7];
    pose7(k->GetPose(), p);
    kf_index[k] = (int)kfs.size(); kfs.push_back(k);
    poses.insert(poses.end(), p, p + 7);
    fixed.push_back(k->mnId == 0 ? 1 : 0);                          // :491
    if (k->mnId > maxKFid) maxKFid = k->mnId;
  }
  std::vector<MapPoint*> mps;                                       // the included points (vbNotIncludedMP[i] == false)
  for (MapPoint* pMP : vpMP) {
    if (pMP->isBad()) continue;
    const int i = (int)mps.size();
    const size_t e0 = e_pose.size();
    for (const auto& ob : pMP->GetObservations()) {
      KeyFrame* k = ob.first;
      if (k->isBad() || k->mnId > maxKFid) continue;                // :520
      const auto it = kf_index.find(k);
      if (it == kf_index.end()) continue;                           // no vertex of that id (the reference would hand g2o a null vertex)
      if (k->mvKeyRays[ob.second](2) < cam->GetCosFovTh()) continue;            // :525
      const cv::KeyPoint& kp = k->mvKeys[ob.second];
      double u, v;
      cam->GetPosInFace(u, v, (double)kp.pt.x, (double)kp.pt.y);
      e_pose.push_back(it->second); e_point.push_back(i); e_obs.push_back(u); e_obs.push_back(v);
      e_inv.push_back(k->mvInvLevelSigma2[kp.octave]); e_face.push_back((int8_t)cam->FaceInCubemap(kp.pt));
    }
    if (e_pose.size() == e0) continue;                              // :559-563: removed from the graph, never written
    mps.push_back(pMP);
    const cv::Mat x = pMP->GetWorldPos();
    for (int k = 0; k < 3; ++k) points.push_back(x.at<float>(k));
  }
  const int K = (int)kfs.size(), P = (int)mps.size(), E = (int)e_pose.size();
  if (K > 0 && E > 0) {
    cms_ba* ba = nullptr;
    check(cms_ba_create(&ba, g_device, K, poses.data(), fixed.data(), P, points.data(), E, e_pose.data(), e_point.data(), e_obs.data(), e_inv.data(), e_face.data(),
                        cam->Get_fx(), cam->Get_fy(), cam->Get_cx(), cam->Get_cy()), "cms_ba_create");
    int rc = cms_ba_optimize_global(ba, nIterations, bRobust ? 1 : 0, reinterpret_cast<const volatile uint8_t*>(pbStopFlag), nullptr);      // :570-572
    if (rc >= 0) { const int rr = cms_ba_read(ba, poses.data(), points.data(), nullptr); if (rr < 0) rc = rr; }
    cms_ba_destroy(ba);
    check(rc, "cms_ba_optimize_global");
  }
  // ---- :577-619
  for (int j = 0; j < K; ++j) {
    if (nLoopKF == 0) kfs[j]->SetPose(toMat(&poses[(size_t)j * 7]));
    else {
      kfs[j]->mTcwGBA.create(4, 4, CV_32F);
      toMat(&poses[(size_t)j * 7]).copyTo(kfs[j]->mTcwGBA);
      kfs[j]->mnBAGlobalForKF = nLoopKF;
    }
  }
  for (int i = 0; i < P; ++i) {
    if (nLoopKF == 0) {
      cv::Mat x(3, 1, CV_32F);
      for (int k = 0; k < 3; ++k) x.at<float>(k) = (float)points[(size_t)i * 3 + k];
      mps[i]->SetWorldPos(x);
      mps[i]->UpdateNormalAndDepth();
    } else {
      mps[i]->mPosGBA.create(3, 1, CV_32F);
      for (int k = 0; k < 3; ++k) mps[i]->mPosGBA.at<float>(k) = (float)points[(size_t)i * 3 + k];
      mps[i]->mnBAGlobalForKF = nLoopKF;
    }
  }
}

// ------------------------------------------------------------------------------------------------ LocalMapping on resident key frames
namespace {
// The book is read by the tracking thread (SearchByBoW) and written by the mapping thread.  `mu` guards the two containers, and it is also held
// across every host call that refills or updates a slot (cms_kfstore_put_from_frame, cms_kfstore_update) and across a whole search, so a slot a
// search names is never released, refilled or updated while the search runs (the threading contract of cms_kfstore_search_by_bow).
// dev_mp: the map-point row each slot holds on the device, as the bridge last sent it (every upload of a row goes through here), so that
// Hip::BuildCovisibility sends only the entries that changed since
struct StoreBook { std::map<KeyFrame*, int> slot; std::vector<int> free_slots; int max_features = 0; std::map<int, std::vector<int> > dev_mp; std::mutex mu; };
std::map<cms_kfstore*, StoreBook> g_books;      // (std::map: a StoreBook never moves once created)
std::mutex g_books_mutex;
StoreBook& book(cms_kfstore* st) { std::lock_guard<std::mutex> lk(g_books_mutex); return g_books[st]; }
int slot_locked(StoreBook& b, KeyFrame* k) { const auto it = b.slot.find(k); return it == b.slot.end() ? -1 : it->second; }      // b.mu held
int slot_of(StoreBook& b, KeyFrame* k) { std::lock_guard<std::mutex> lk(b.mu); return slot_locked(b, k); }
struct DbBook { std::set<KeyFrame*> in_db; std::mutex mu; };      // which resident key frames are in the store's KeyFrameDatabase (Hip::AddToDatabase)
std::map<cms_kfstore*, DbBook> g_db_books;
std::mutex g_db_books_mutex;
DbBook& db_book(cms_kfstore* st) { std::lock_guard<std::mutex> lk(g_db_books_mutex); return g_db_books[st]; }
void pose_floats(KeyFrame* k, float* R9, float* t3, float* O3) {
  const cv::Mat R = k->GetRotation(), t = k->GetTranslation(), O = k->GetCameraCenter();
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) R9[3 * r + c] = R.at<float>(r, c); t3[r] = t.at<float>(r); O3[r] = O.at<float>(r); }
}
// the map-point slot per key point as the device holds it: the point's id & 0x3FFFFFFF where the key point holds a point that is not bad.  A row names
// an id once (the observation index refuses a row that repeats one): where two key points hold the same point, the one the point itself names
// (GetIndexInKeyFrame) keeps it
void mp_slots(KeyFrame* k, std::vector<int>& mp) {
  const std::vector<MapPoint*> v = k->GetMapPointMatches();
  mp.assign(v.size(), -1);
  std::map<MapPoint*, int> kept;      // the key point that holds the point's id so far
  for (size_t i = 0; i < v.size(); ++i) {
    if (!v[i] || v[i]->isBad()) continue;
    const auto it = kept.find(v[i]);
    if (it != kept.end()) {           // the row would repeat the id: the key point the point names keeps it, else the first one
      if (v[i]->GetIndexInKeyFrame(k) != (int)i) continue;
      mp[(size_t)it->second] = -1;
    }
    kept[v[i]] = (int)i;
    mp[i] = (int)(v[i]->mnId & 0x3FFFFFFF);
  }
}
// a map point as the Fuse search reads it (ORBMatcher.cpp:1140-1175)
void push_point(MapPoint* p, std::vector<float>& pos, std::vector<float>& nrm, std::vector<float>& dmin, std::vector<float>& dmax, std::vector<uint8_t>& desc) {
  const cv::Mat x = p->GetWorldPos(), n = p->GetNormal(), d = p->GetDescriptor();
  for (int k = 0; k < 3; ++k) { pos.push_back(x.at<float>(k)); nrm.push_back(n.at<float>(k)); }
  dmin.push_back(p->GetMinDistanceInvariance()); dmax.push_back(p->GetMaxDistanceInvariance());      // (the store's context runs in distance-bounds mode 1, see CreateContext)
  desc.insert(desc.end(), d.data, d.data + 32);
}
}  // namespace

cms_kfstore* CreateKeyFrameStore(cms_ctx* mappingCtx, int maxKeyFrames, int maxFeatures) {
  cms_kfstore* st = nullptr;
  check(cms_kfstore_create(&st, mappingCtx, maxKeyFrames, maxFeatures, 4096), "cms_kfstore_create");
  StoreBook& b = book(st);
  std::lock_guard<std::mutex> lk(b.mu);
  b.max_features = maxFeatures;
  for (int s = maxKeyFrames - 1; s >= 0; --s) b.free_slots.push_back(s);
  return st;
}

int ProcessNewKeyFrame(cms_kfstore* store, cms_ctx* frameCtx, KeyFrame* pKF) {
  StoreBook& b = book(store);
  std::lock_guard<std::mutex> lk(b.mu);      // (to the end: the book entry appears together with the put, and no search runs on a slot being refilled)
  int slot = slot_locked(b, pKF);
  if (slot < 0) {
    if (b.free_slots.empty()) throw std::runtime_error("Hip::ProcessNewKeyFrame: the key-frame store is full");
    slot = b.free_slots.back(); b.free_slots.pop_back(); b.slot[pKF] = slot;
  }
  // mFeatVec (KeyFrame::ComputeBoW, LocalMapping.cpp:62): node id -> feature indices, std::map order
  std::vector<int> node_id, node_off(1, 0), node_feat, mp;
  for (const auto& nf : pKF->mFeatVec) {
    node_id.push_back((int)nf.first);
    for (unsigned f : nf.second) node_feat.push_back((int)f);
    node_off.push_back((int)node_feat.size());
  }
  mp_slots(pKF, mp);
  float R[9], t[3], O[3];
  pose_floats(pKF, R, t, O);
  check(cms_kfstore_put_from_frame(store, slot, frameCtx, 0, pKF->N, R, t, O, pKF->ComputeSceneMedianDepth(2), mp.data(), (int)node_id.size(), node_id.data(),
                                   node_off.data(), node_feat.data()), "cms_kfstore_put_from_frame");
  b.dev_mp[slot] = mp;
  return slot;
}

void ReleaseKeyFrame(cms_kfstore* store, KeyFrame* pKF) {
  StoreBook& b = book(store);
  std::lock_guard<std::mutex> lk(b.mu);
  const auto it = b.slot.find(pKF);
  if (it == b.slot.end()) return;
  {      // a key frame that leaves the store leaves its database
    DbBook& d = db_book(store);
    std::lock_guard<std::mutex> lk2(d.mu);
    if (d.in_db.erase(pKF)) check(cms_kfdb_erase(store, 1, &it->second), "cms_kfdb_erase");
  }
  b.dev_mp.erase(it->second);
  b.free_slots.push_back(it->second);
  b.slot.erase(it);
}

namespace {
// mps == NULL: every neighbour's median depth is computed on the host and handed over; otherwise ONE cms_kfstore_scene_median_depth call with
// store = 1 for the current key frame and its neighbours, from the rows just sent and the table's positions
int create_new_map_points(cms_kfstore* store, cms_mpstore* mps, KeyFrame* pCurrentKF, Map* pMap, std::vector<MapPoint*>& newPoints) {
  StoreBook& b = book(store);
  const int cur = slot_of(b, pCurrentKF);
  if (cur < 0) throw std::runtime_error("Hip::CreateNewMapPoints: the current key frame is not resident (Hip::ProcessNewKeyFrame first)");
  std::vector<KeyFrame*> neigh;                                    // GetBestCovisibilityKeyFrames(20), the resident ones, in covisibility order
  std::vector<int> neigh_slot;
  for (KeyFrame* k : pCurrentKF->GetBestCovisibilityKeyFrames(20)) {
    const int s = slot_of(b, k);
    if (s < 0 || k->isBad()) continue;
    // poses, median depths and map-point slots may have changed since the key frame entered the store (local BA, Fuse, culling)
    float R[9], t[3], O[3]; std::vector<int> mp;
    pose_floats(k, R, t, O); mp_slots(k, mp);
    const float md = mps ? 0.0f : k->ComputeSceneMedianDepth(2);
    {
      std::lock_guard<std::mutex> lk(b.mu);
      check(cms_kfstore_update(store, s, R, t, O, mps ? nullptr : &md, mp.data()), "cms_kfstore_update");
      b.dev_mp[s] = mp;
    }
    neigh.push_back(k); neigh_slot.push_back(s);
  }
  {
    float R[9], t[3], O[3]; std::vector<int> mp;
    pose_floats(pCurrentKF, R, t, O); mp_slots(pCurrentKF, mp);
    std::lock_guard<std::mutex> lk(b.mu);
    check(cms_kfstore_update(store, cur, R, t, O, nullptr, mp.data()), "cms_kfstore_update");
    b.dev_mp[cur] = mp;
  }
  if (neigh.empty()) return 0;
  if (mps) {
    std::vector<int> slots(1, cur);
    slots.insert(slots.end(), neigh_slot.begin(), neigh_slot.end());
    std::vector<float> depth(slots.size());
    std::vector<int> n_depths(slots.size());
    check(cms_kfstore_scene_median_depth(store, mps, (int)slots.size(), slots.data(), 2, 1, depth.data(), n_depths.data()), "cms_kfstore_scene_median_depth");
  }
  const int cap = pCurrentKF->N;
  const int neigh_off[2] = {0, (int)neigh.size()};
  int n_new = 0;
  std::vector<int> o_neigh(cap), o_idx1(cap), o_idx2(cap);
  std::vector<float> o_x((size_t)cap * 3);
  check(cms_kfstore_create_new_map_points(store, 1, &cur, neigh_off, neigh_slot.data(), 0, cap, &n_new, o_neigh.data(), o_idx1.data(), o_idx2.data(), o_x.data()),
        "cms_kfstore_create_new_map_points");
  for (int i = 0; i < n_new; ++i) {                                // LocalMapping.cpp:359-381, in the reference's creation order
    KeyFrame* pKF2 = neigh[o_neigh[i]];
    cv::Mat x3D(3, 1, CV_32F);
    for (int k = 0; k < 3; ++k) x3D.at<float>(k) = o_x[(size_t)i * 3 + k];
    MapPoint* pMP = new MapPoint(x3D, pCurrentKF, pMap);
    pMP->AddObservation(pCurrentKF, o_idx1[i]);
    pMP->AddObservation(pKF2, o_idx2[i]);
    pCurrentKF->AddMapPoint(pMP, o_idx1[i]);
    pKF2->AddMapPoint(pMP, o_idx2[i]);
    pMP->ComputeDistinctiveDescriptors();
    pMP->UpdateNormalAndDepth();
    pMap->AddMapPoint(pMP);
    newPoints.push_back(pMP);
  }
  return n_new;
}
}  // namespace
int CreateNewMapPoints(cms_kfstore* store, KeyFrame* pCurrentKF, Map* pMap, std::vector<MapPoint*>& newPoints) {
  return create_new_map_points(store, nullptr, pCurrentKF, pMap, newPoints);
}
int CreateNewMapPoints(cms_kfstore* store, cms_mpstore* mps, KeyFrame* pCurrentKF, Map* pMap, std::vector<MapPoint*>& newPoints) {
  return create_new_map_points(store, mps, pCurrentKF, pMap, newPoints);
}

namespace {
void search_in_neighbors_fuse(cms_kfstore* store, KeyFrame* pCurrentKF, cms_mpstore* mps, std::vector<MapPoint*>* replaced);
bool row_ready(cms_mpstore* mps, MapPoint* p);
}
void SearchInNeighbors(cms_kfstore* store, KeyFrame* pCurrentKF) {
  search_in_neighbors_fuse(store, pCurrentKF, nullptr, nullptr);
  pCurrentKF->UpdateConnections();
}
namespace {
// LocalMapping.cpp:388-463: everything of SearchInNeighbors but the final UpdateConnections.  mps (NULL: the points' attributes travel as host arrays):
// the search takes ids into the table, points without a refreshed row stay out of the sets, `replaced` receives the points Replace made bad, and the
// update of the current key frame's points (:449-463) is left to the caller, which refreshes their rows
void search_in_neighbors_fuse(cms_kfstore* store, KeyFrame* pCurrentKF, cms_mpstore* mps, std::vector<MapPoint*>* replaced) {
  StoreBook& b = book(store);
  const int cur = slot_of(b, pCurrentKF);
  if (cur < 0) throw std::runtime_error("Hip::SearchInNeighbors: the current key frame is not resident");
  // ---- target key frames: neighbours and second neighbours (LocalMapping.cpp:391-412), the resident ones
  std::vector<KeyFrame*> targets;
  for (KeyFrame* k : pCurrentKF->GetBestCovisibilityKeyFrames(20)) {
    if (k->isBad() || k->mnFuseTargetForKF == pCurrentKF->mnId) continue;
    targets.push_back(k);
    k->mnFuseTargetForKF = pCurrentKF->mnId;
    for (KeyFrame* k2 : k->GetBestCovisibilityKeyFrames(5)) {
      if (k2->isBad() || k2->mnFuseTargetForKF == pCurrentKF->mnId || k2->mnId == pCurrentKF->mnId) continue;
      targets.push_back(k2);
    }
  }
  std::vector<KeyFrame*> tk;
  for (KeyFrame* k : targets) if (slot_of(b, k) >= 0) tk.push_back(k);
  if (tk.empty()) return;
  // ---- set 0: the current key frame's map points (into every target); set 1: the targets' map points, first appearance (into the current key frame)
  std::vector<MapPoint*> set0, set1;
  for (MapPoint* p : pCurrentKF->GetMapPointMatches())
    if (p && (!mps || row_ready(mps, p))) set0.push_back(p);                                // (ORBMatcher::Fuse skips null / bad points itself: the skip flags below)
  for (KeyFrame* k : tk)
    for (MapPoint* p : k->GetMapPointMatches()) {
      if (!p || p->isBad() || p->mnFuseCandidateForKF == pCurrentKF->mnId) continue;        // LocalMapping.cpp:432-447
      p->mnFuseCandidateForKF = pCurrentKF->mnId;
      if (!mps || row_ready(mps, p)) set1.push_back(p);
    }
  std::vector<float> pos, nrm, dmin, dmax;
  std::vector<uint8_t> desc;
  std::vector<int> ids;
  if (mps) {
    for (MapPoint* p : set0) ids.push_back((int)p->mnId);
    for (MapPoint* p : set1) ids.push_back((int)p->mnId);
  } else {
    for (MapPoint* p : set0) push_point(p, pos, nrm, dmin, dmax, desc);
    for (MapPoint* p : set1) push_point(p, pos, nrm, dmin, dmax, desc);
  }
  const int set_off[3] = {0, (int)set0.size(), (int)(set0.size() + set1.size())};
  // ---- jobs: set 0 into every target, set 1 into the current key frame; an entry is skipped like ORBMatcher.cpp:1143-1147 skips it
  std::vector<int> job_slot, job_set;
  std::vector<uint8_t> skip;
  for (KeyFrame* k : tk) {
    job_slot.push_back(slot_of(b, k)); job_set.push_back(0);
    for (MapPoint* p : set0) skip.push_back((p->isBad() || p->IsInKeyFrame(k)) ? 1 : 0);
  }
  job_slot.push_back(cur); job_set.push_back(1);
  for (MapPoint* p : set1) skip.push_back((p->isBad() || p->IsInKeyFrame(pCurrentKF)) ? 1 : 0);
  // the searched key frames' map-point slots as they are NOW (the search only needs the key points; the decisions below read the live objects)
  std::vector<int> best_idx(skip.size()), best_dist(skip.size());
  if (mps)
    check(cms_kfstore_fuse_search_sets_ids(store, mps, 2, set_off, ids.data(), (int)job_slot.size(), job_slot.data(), job_set.data(), skip.data(), 3.0f,
                                           best_idx.data(), best_dist.data()), "cms_kfstore_fuse_search_sets_ids");
  else
    check(cms_kfstore_fuse_search_sets(store, 2, set_off, pos.data(), nrm.data(), dmin.data(), dmax.data(), desc.data(), (int)job_slot.size(), job_slot.data(),
                                       job_set.data(), skip.data(), 3.0f, best_idx.data(), best_dist.data()), "cms_kfstore_fuse_search_sets");
  // ---- the decisions, job after job and point after point in the reference's order (ORBMatcher.cpp:1213-1236).  A point that an earlier job of this
  // call added to / replaced in a later job's key frame is re-checked here exactly like the reference's sequential Fuse calls would see it
  size_t e = 0;
  for (size_t j = 0; j < job_slot.size(); ++j) {
    KeyFrame* pKF = j < tk.size() ? tk[j] : pCurrentKF;
    const std::vector<MapPoint*>& pts = j < tk.size() ? set0 : set1;
    for (size_t i = 0; i < pts.size(); ++i, ++e) {
      MapPoint* pMP = pts[i];
      if (best_idx[e] < 0 || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
      MapPoint* pMPinKF = pKF->GetMapPoint(best_idx[e]);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) {
          MapPoint* gone = pMPinKF->Observations() > pMP->Observations() ? pMP : pMPinKF;
          gone->Replace(gone == pMP ? pMPinKF : pMP);
          if (replaced) replaced->push_back(gone);
        }
      } else {
        pMP->AddObservation(pKF, best_idx[e]);
        pKF->AddMapPoint(pMP, best_idx[e]);
      }
    }
  }
  // ---- update points and connections (LocalMapping.cpp:449-465)
  if (mps) return;                                                 // (the caller refreshes the rows once the index has seen the fusion)
  for (MapPoint* p : pCurrentKF->GetMapPointMatches())
    if (p && !p->isBad()) { p->ComputeDistinctiveDescriptors(); p->UpdateNormalAndDepth(); }
}
}  // namespace

// ------------------------------------------------------------------------------------------------ Covisibility on the device
namespace {
// the members of a cms_covis as of its last build, and the map points behind the ids of their rows
struct CovisBook { std::vector<KeyFrame*> members; std::map<KeyFrame*, int> pos; std::map<int, MapPoint*> point; std::mutex mu; };
std::map<cms_covis*, CovisBook> g_covis_books;
std::mutex g_covis_books_mutex;
CovisBook& covis_book(cms_covis* cv) { std::lock_guard<std::mutex> lk(g_covis_books_mutex); return g_covis_books[cv]; }
int member_of(CovisBook& c, KeyFrame* k) { const auto it = c.pos.find(k); return it == c.pos.end() ? -1 : it->second; }      // c.mu held
}  // namespace

cms_covis* CreateCovisibility(cms_kfstore* store, int maxKeyFrames) {
  cms_covis* cv = nullptr;
  check(cms_covis_create(&cv, store, maxKeyFrames), "cms_covis_create");
  return cv;
}

void BuildCovisibility(cms_kfstore* store, cms_covis* covis, const std::vector<KeyFrame*>& vpKFs) {
  StoreBook& b = book(store);
  CovisBook& c = covis_book(covis);
  std::lock_guard<std::mutex> lkc(c.mu);
  c.members.clear(); c.pos.clear(); c.point.clear();
  std::vector<int> slots, up_slot, up_feat, up_mp;      // the members; the (slot, feature, id) entries that differ from what the device holds
  std::lock_guard<std::mutex> lk(b.mu);
  for (KeyFrame* k : vpKFs) {
    if (!k || k->isBad() || c.pos.count(k)) continue;
    const int s = slot_locked(b, k);
    if (s < 0) continue;
    std::vector<int> mp;
    mp_slots(k, mp);
    const std::vector<MapPoint*> v = k->GetMapPointMatches();
    for (size_t i = 0; i < v.size(); ++i) if (mp[i] >= 0) c.point[mp[i]] = v[i];
    std::vector<int>& have = b.dev_mp[s];
    if (have.size() != mp.size()) {                     // a row the bridge has no record of: the whole row, once
      check(cms_kfstore_update(store, s, nullptr, nullptr, nullptr, nullptr, mp.data()), "cms_kfstore_update");
    } else {
      for (size_t i = 0; i < mp.size(); ++i)
        if (mp[i] != have[i]) { up_slot.push_back(s); up_feat.push_back((int)i); up_mp.push_back(mp[i]); }
    }
    have.swap(mp);
    c.pos[k] = (int)c.members.size(); c.members.push_back(k); slots.push_back(s);
  }
  // Fuse's Replace, MapPointCulling, new points: a handful of entries in many key frames -- ONE asynchronous scatter, no copy and no wait per key frame
  if (!up_slot.empty())
    check(cms_kfstore_update_map_points(store, (int)up_slot.size(), up_slot.data(), up_feat.data(), up_mp.data()), "cms_kfstore_update_map_points");
  check(cms_covis_build(covis, (int)slots.size(), slots.data()), "cms_covis_build");
}

Connections UpdateConnections(cms_kfstore* store, cms_covis* covis, KeyFrame* pKF) {
  (void)store;
  CovisBook& c = covis_book(covis);
  std::lock_guard<std::mutex> lk(c.mu);
  const int job = member_of(c, pKF);
  if (job < 0) throw std::runtime_error("Hip::UpdateConnections: the key frame is not a member of the last Hip::BuildCovisibility");
  const size_t M = c.members.size();
  std::vector<int> w(M), order(M);
  int n = 0;
  check(cms_covis_connections(covis, 1, &job, 15, w.data(), order.data(), &n), "cms_covis_connections");
  Connections out;
  for (size_t m = 0; m < M; ++m) if (w[m] > 0) out.weights[c.members[m]] = w[m];      // KFcounter (:338-346)
  for (int i = 0; i < n; ++i) {
    KeyFrame* k = c.members[(size_t)order[(size_t)i]];
    k->AddConnection(pKF, w[(size_t)order[(size_t)i]]);                               // :370, :377
    out.ordered.push_back(k); out.orderedWeights.push_back(w[(size_t)order[(size_t)i]]);
  }
  return out;
}

Connections SearchInNeighbors(cms_kfstore* store, cms_covis* covis, KeyFrame* pCurrentKF) {
  search_in_neighbors_fuse(store, pCurrentKF, nullptr, nullptr);
  return UpdateConnections(store, covis, pCurrentKF);
}

std::vector<KeyFrame*> KeyFrameCulling(cms_kfstore* store, cms_covis* covis, KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpNotErase) {
  (void)store;
  CovisBook& c = covis_book(covis);
  std::vector<KeyFrame*> cand;
  std::vector<int> jobs;
  std::vector<uint8_t> erasable;
  {
    std::lock_guard<std::mutex> lk(c.mu);
    const std::set<KeyFrame*> keep(vpNotErase.begin(), vpNotErase.end());
    for (KeyFrame* k : pCurrentKF->GetVectorCovisibleKeyFrames()) {
      if (k->mnId == 0) continue;                                                     // :572
      const int m = member_of(c, k);
      if (m < 0) continue;
      cand.push_back(k); jobs.push_back(m); erasable.push_back(keep.count(k) ? 0 : 1);
    }
  }
  std::vector<KeyFrame*> culled;
  if (cand.empty()) return culled;
  const int off[2] = {0, (int)jobs.size()};
  std::vector<int> n_mps(jobs.size()), n_red(jobs.size());
  std::vector<uint8_t> red(jobs.size());
  check(cms_covis_culling(covis, 1, off, jobs.data(), erasable.data(), 3, n_mps.data(), n_red.data(), red.data()), "cms_covis_culling");
  for (size_t i = 0; i < cand.size(); ++i)
    if (red[i]) { cand[i]->SetBadFlag(); culled.push_back(cand[i]); }                 // :616-617 (SetBadFlag honours mbNotErase itself)
  return culled;
}

void UpdateLocalMap(cms_covis* covis, cms_ctx* frameCtx, Frame& F, std::vector<KeyFrame*>& vpLocalKeyFrames, KeyFrame*& pKFmax, std::vector<MapPoint*>& vpLocalMapPoints) {
  CovisBook& c = covis_book(covis);
  std::lock_guard<std::mutex> lk(c.mu);
  vpLocalKeyFrames.clear(); vpLocalMapPoints.clear(); pKFmax = NULL;
  // ---- the votes (Tracking.cpp:885-901)
  std::vector<int> ids;
  for (int i = 0; i < F.N; ++i) {
    MapPoint* p = F.mvpMapPoints[i];
    if (!p) continue;
    if (p->isBad()) { F.mvpMapPoints[i] = NULL; continue; }
    ids.push_back((int)(p->mnId & 0x3FFFFFFF));
  }
  const size_t M = c.members.size();
  std::vector<int> votes(M + 1, 0);
  const int id_off[2] = {0, (int)ids.size()};
  ids.push_back(0);
  check(cms_covis_votes(covis, frameCtx, 1, id_off, ids.data(), votes.data()), "cms_covis_votes");
  // ---- :903-928 in member order, then the neighbours of :930-981 on the pointer graph
  int max = 0;
  std::set<KeyFrame*> in;
  for (size_t m = 0; m < M; ++m) {
    if (votes[m] == 0 || c.members[m]->isBad()) continue;
    if (votes[m] > max) { max = votes[m]; pKFmax = c.members[m]; }
    vpLocalKeyFrames.push_back(c.members[m]); in.insert(c.members[m]);
  }
  if (vpLocalKeyFrames.empty()) return;                                               // keyframeCounter.empty() (:903)
  for (size_t i = 0; i < vpLocalKeyFrames.size(); ++i) {
    if (vpLocalKeyFrames.size() > 80) break;
    KeyFrame* pKF = vpLocalKeyFrames[i];
    for (KeyFrame* n : pKF->GetBestCovisibilityKeyFrames(10))
      if (!n->isBad() && in.insert(n).second) { vpLocalKeyFrames.push_back(n); break; }
    for (KeyFrame* ch : pKF->GetChilds())
      if (!ch->isBad() && in.insert(ch).second) { vpLocalKeyFrames.push_back(ch); break; }
    KeyFrame* pParent = pKF->GetParent();
    if (pParent && in.insert(pParent).second) { vpLocalKeyFrames.push_back(pParent); break; }      // (:971-978: the reference's break leaves the loop)
  }
  // ---- UpdateLocalPoints (:857-877) over the local key frames that are members
  std::vector<int> kfs;
  size_t cap = 1;
  for (KeyFrame* k : vpLocalKeyFrames) { const int m = member_of(c, k); if (m >= 0) { kfs.push_back(m); cap += (size_t)k->N; } }
  const int kf_off[2] = {0, (int)kfs.size()};
  kfs.push_back(0);
  std::vector<int> out(cap);
  int n = 0;
  check(cms_covis_local_points(covis, frameCtx, 1, kf_off, kfs.data(), (int)cap, out.data(), &n), "cms_covis_local_points");
  for (int i = 0; i < n; ++i) {
    const auto it = c.point.find(out[(size_t)i]);
    if (it != c.point.end() && !it->second->isBad()) vpLocalMapPoints.push_back(it->second);
  }
}

// ------------------------------------------------------------------------------------------------ Map points on the device
namespace {
// a table's store and capacity, and which rows hold what: `set` by Hip::SetMapPoints, `ready` once a refresh has given the row a descriptor AND
// normal and depth (what the two consumers ask for).  Erased rows leave both.
struct MpBook { cms_kfstore* store = nullptr; int max_points = 0; std::set<int> set, has_desc, has_normal; std::mutex mu; };
std::map<cms_mpstore*, MpBook> g_mp_books;
std::mutex g_mp_books_mutex;
MpBook& mp_book(cms_mpstore* mps) { std::lock_guard<std::mutex> lk(g_mp_books_mutex); return g_mp_books[mps]; }
// the row of a map point, -1: its mnId does not fit the table
int row_of(const MpBook& m, MapPoint* p) { return p->mnId < (long unsigned int)m.max_points ? (int)p->mnId : -1; }
bool row_ready(cms_mpstore* mps, MapPoint* p) {
  MpBook& m = mp_book(mps);
  std::lock_guard<std::mutex> lk(m.mu);
  const int r = row_of(m, p);
  return r >= 0 && !p->isBad() && m.has_desc.count(r) && m.has_normal.count(r);
}
}  // namespace

cms_mpstore* CreateMapPointStore(cms_kfstore* store, int maxPoints) {
  cms_mpstore* mps = nullptr;
  check(cms_mpstore_create(&mps, store, maxPoints), "cms_mpstore_create");
  MpBook& m = mp_book(mps);
  std::lock_guard<std::mutex> lk(m.mu);
  m.store = store; m.max_points = maxPoints;
  return mps;
}

int SetMapPoints(cms_mpstore* mps, const std::vector<MapPoint*>& vpMPs) {
  MpBook& m = mp_book(mps);
  std::lock_guard<std::mutex> lk(m.mu);
  StoreBook& b = book(m.store);
  std::vector<int> ids, ref;
  std::vector<float> pos;
  std::set<int> named;
  for (MapPoint* p : vpMPs) {
    if (!p || p->isBad()) continue;
    const int r = row_of(m, p);
    if (r < 0) throw std::runtime_error("Hip::SetMapPoints: a map point's mnId is beyond the table (Hip::CreateMapPointStore's maxPoints)");
    KeyFrame* pRef = p->GetReferenceKeyFrame();
    const int s = pRef ? slot_of(b, pRef) : -1;
    if (s < 0 || !named.insert(r).second) continue;               // (the reference key frame is not resident; or the point is listed twice)
    const cv::Mat x = p->GetWorldPos();
    ids.push_back(r); ref.push_back(s);
    for (int k = 0; k < 3; ++k) pos.push_back(x.at<float>(k));
  }
  if (ids.empty()) return 0;
  check(cms_mpstore_set(mps, (int)ids.size(), ids.data(), pos.data(), ref.data()), "cms_mpstore_set");
  m.set.insert(ids.begin(), ids.end());
  return (int)ids.size();
}

void EraseMapPoints(cms_mpstore* mps, const std::vector<MapPoint*>& vpMPs) {
  MpBook& m = mp_book(mps);
  std::lock_guard<std::mutex> lk(m.mu);
  std::vector<int> ids;
  std::set<int> named;
  for (MapPoint* p : vpMPs) {
    if (!p) continue;
    const int r = row_of(m, p);
    if (r >= 0 && m.set.count(r) && named.insert(r).second) ids.push_back(r);
  }
  if (ids.empty()) return;
  check(cms_mpstore_erase(mps, (int)ids.size(), ids.data()), "cms_mpstore_erase");
  for (int r : ids) { m.set.erase(r); m.has_desc.erase(r); m.has_normal.erase(r); }
}

std::vector<MapPointAttributes> RefreshMapPoints(cms_mpstore* mps, cms_covis* covis, const std::vector<MapPoint*>& vpMPs, int what) {
  MpBook& m = mp_book(mps);
  std::lock_guard<std::mutex> lk(m.mu);
  std::vector<MapPointAttributes> out;
  std::vector<int> ids;
  std::set<int> named;
  for (MapPoint* p : vpMPs) {
    if (!p || p->isBad()) continue;
    const int r = row_of(m, p);
    if (r < 0 || !m.set.count(r) || !named.insert(r).second) continue;
    MapPointAttributes a;
    a.pMP = p; a.status = 0; a.minDistance = 0.0f; a.maxDistance = 0.0f;
    out.push_back(a); ids.push_back(r);
  }
  const size_t n = ids.size();
  if (n == 0) return out;
  std::vector<uint8_t> status(n), desc(32 * n);
  std::vector<float> nrm(3 * n), dmin(n), dmax(n);
  check(cms_mpstore_refresh(mps, covis, (int)n, ids.data(), what, status.data()), "cms_mpstore_refresh");
  check(cms_mpstore_fetch(mps, (int)n, ids.data(), nullptr, nrm.data(), dmin.data(), dmax.data(), desc.data(), nullptr, nullptr), "cms_mpstore_fetch");
  for (size_t i = 0; i < n; ++i) {
    MapPointAttributes& a = out[i];
    a.status = status[i];
    a.descriptor = cv::Mat(1, 32, CV_8U);
    std::memcpy(a.descriptor.data, &desc[32 * i], 32);
    a.normal = cv::Mat(3, 1, CV_32F);
    for (int k = 0; k < 3; ++k) a.normal.at<float>(k) = nrm[3 * i + k];
    a.minDistance = dmin[i]; a.maxDistance = dmax[i];
    if (status[i] == 0) {
      if (what & CMS_MP_DESCRIPTOR) m.has_desc.insert(ids[i]);
      if (what & CMS_MP_NORMAL_DEPTH) m.has_normal.insert(ids[i]);
    }
  }
  return out;
}

int SearchLocalPoints(cms_ctx* ctx, cms_mpstore* mps, Frame& F, const std::vector<MapPoint*>& vpMapPoints, float th) {
  // the caller (Tracking::SearchLocalPoints, Tracking.cpp:797-822) has removed the points already matched in the frame and the bad ones
  const int n = (int)vpMapPoints.size();
  std::vector<float> px(n), py(n), vc(n);
  std::vector<uint8_t> inview(n);
  std::vector<int> ids(n), level(n), match(n);
  {
    MpBook& m = mp_book(mps);
    std::lock_guard<std::mutex> lk(m.mu);
    for (int i = 0; i < n; ++i) {
      ids[i] = row_of(m, vpMapPoints[i]);
      if (ids[i] < 0) throw std::runtime_error("Hip::SearchLocalPoints: a map point's mnId is beyond the table");
    }
  }
  float pose15[15];
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) pose15[3 * r + c] = F.mTcw.at<float>(r, c); pose15[9 + r] = F.mTcw.at<float>(r, 3); }
  const cv::Mat Ow = F.GetCameraCenter();
  for (int k = 0; k < 3; ++k) pose15[12 + k] = Ow.at<float>(k);
  std::vector<int> kp_mp(F.N);
  for (int i = 0; i < F.N; ++i) { MapPoint* p = F.mvpMapPoints[i]; kp_mp[i] = (p && p->Observations() > 0) ? (1 << 30) : -1; }   // ORBMatcher.cpp:91-95
  int nm = 0;
  check(cms_search_local_points_ids(ctx, 0, pose15, mps, n, ids.data(), 0.5f, th, 0.8f, ORBMatcher::TH_HIGH, F.N, kp_mp.data(), inview.data(), px.data(), py.data(),
                                    level.data(), vc.data(), match.data(), &nm, nullptr), "cms_search_local_points_ids");
  for (int i = 0; i < n; ++i) {                                    // what Frame::isInFrustum leaves on the MapPoint (Frame.cpp:199-248) ...
    MapPoint* p = vpMapPoints[i];
    p->mbTrackInView = inview[i] != 0;
    if (!inview[i]) continue;
    p->mTrackProjX = px[i]; p->mTrackProjY = py[i]; p->mnTrackScaleLevel = level[i]; p->mTrackViewCos = vc[i];
    p->IncreaseVisible();                                          // Tracking.cpp:829
    if (match[i] >= 0) F.mvpMapPoints[match[i]] = p;               // ... and what the matcher leaves in the frame (ORBMatcher.cpp:121)
  }
  return nm;
}

Connections SearchInNeighbors(cms_kfstore* store, cms_covis* covis, cms_mpstore* mps, KeyFrame* pCurrentKF, std::vector<MapPointAttributes>& refreshed) {
  std::vector<MapPoint*> replaced;
  search_in_neighbors_fuse(store, pCurrentKF, mps, &replaced);
  EraseMapPoints(mps, replaced);
  std::vector<KeyFrame*> members;
  { CovisBook& c = covis_book(covis); std::lock_guard<std::mutex> lk(c.mu); members = c.members; }
  BuildCovisibility(store, covis, members);                        // the index sees the fusion: AddObservation, Replace
  std::vector<MapPoint*> mine;
  for (MapPoint* p : pCurrentKF->GetMapPointMatches()) if (p && !p->isBad()) mine.push_back(p);      // LocalMapping.cpp:452-463
  SetMapPoints(mps, mine);                                         // (Replace may have moved mpRefKF)
  refreshed = RefreshMapPoints(mps, covis, mine, CMS_MP_DESCRIPTOR | CMS_MP_NORMAL_DEPTH);
  return UpdateConnections(store, covis, pCurrentKF);
}

void UpdateKeyFramePoses(cms_kfstore* store, const std::vector<KeyFrame*>& vpKFs) {
  StoreBook& b = book(store);
  std::vector<int> slots;
  std::vector<float> R, t, O;
  for (KeyFrame* k : vpKFs) {
    const int s = slot_of(b, k);
    if (s < 0) continue;
    float r9[9], t3[3], o3[3];
    pose_floats(k, r9, t3, o3);
    slots.push_back(s); R.insert(R.end(), r9, r9 + 9); t.insert(t.end(), t3, t3 + 3); O.insert(O.end(), o3, o3 + 3);
  }
  if (!slots.empty()) check(cms_kfstore_update_poses(store, (int)slots.size(), slots.data(), R.data(), t.data(), O.data()), "cms_kfstore_update_poses");
}

// Optimizer::LocalBundleAdjustment with the window assembled on the device (cms_covis_local_ba_windows): no walk over observations on the host
void LocalBundleAdjustment(cms_kfstore* store, cms_covis* covis, cms_mpstore* mps, KeyFrame* pKF, bool* pbStopFlag, Map* pMap) {
  CamModelGeneral* cam = CamModelGeneral::GetCamera();
  CovisBook& c = covis_book(covis);
  std::vector<KeyFrame*> members;
  std::map<int, MapPoint*> point;
  std::vector<int> local;
  int first = -1;
  size_t cap_points = 1;
  {
    std::lock_guard<std::mutex> lk(c.mu);
    members = c.members; point = c.point;
    const int m0 = member_of(c, pKF);
    if (m0 < 0) throw std::runtime_error("Hip::LocalBundleAdjustment: the key frame is not a member of the last Hip::BuildCovisibility");
    std::set<int> listed;
    local.push_back(m0); listed.insert(m0);                        // lLocalKeyFrames (Optimizer.cpp:198-207): pKF, then its covisibles in their order
    for (KeyFrame* k : pKF->GetVectorCovisibleKeyFrames()) {
      const int m = member_of(c, k);
      if (m >= 0 && listed.insert(m).second) local.push_back(m);   // (a covisible that is bad or not resident is no member)
    }
    for (size_t m = 0; m < members.size(); ++m) if (members[m]->mnId == 0) first = (int)m;
    for (int m : local) cap_points += members[(size_t)m]->mvKeys.size();
  }
  const int cap_kf = (int)members.size();
  size_t cap_edges = 8 * cap_points;
  cms_ba_window_counts n = {0, 0, 0, 0};
  std::vector<int> kf_member((size_t)cap_kf), point_id(cap_points), e_pose, e_point, e_feat;
  std::vector<double> poses(7 * (size_t)cap_kf), points(3 * cap_points), e_obs, e_inv;
  std::vector<uint8_t> fixed((size_t)cap_kf);
  std::vector<int8_t> e_face;
  const cms_ba_window_job job = {(int)local.size(), local.data(), first};
  for (int attempt = 0; ; ++attempt) {                             // (the number of edges is known after the first call: at most one more)
    e_pose.resize(cap_edges); e_point.resize(cap_edges); e_feat.resize(cap_edges); e_obs.resize(2 * cap_edges); e_inv.resize(cap_edges); e_face.resize(cap_edges);
    const int rc = cms_covis_local_ba_windows(covis, mps, 1, &job, cap_kf, (int)cap_points, (int)cap_edges, &n, kf_member.data(), point_id.data(), poses.data(), fixed.data(),
                                              points.data(), e_pose.data(), e_point.data(), e_obs.data(), e_inv.data(), e_face.data(), e_feat.data());
    if (rc == CMS_OK) break;
    if (rc != CMS_ERR_OVERFLOW || attempt > 0 || n.K > cap_kf || (size_t)n.P > cap_points) check(rc, "cms_covis_local_ba_windows");
    cap_edges = (size_t)n.E;
  }
  const int K = n.K, P = n.P, E = n.E;
  if (E == 0) return;
  std::vector<uint8_t> erase((size_t)E, 0);
  cms_ba_stats st;
  const int rc = cms_ba_run(g_device, K, poses.data(), fixed.data(), P, points.data(), E, e_pose.data(), e_point.data(), e_obs.data(), e_inv.data(), e_face.data(),
                            cam->Get_fx(), cam->Get_fy(), cam->Get_cx(), cam->Get_cy(), 5, 10, reinterpret_cast<const volatile uint8_t*>(pbStopFlag), erase.data(), &st);
  check(rc, "cms_ba_run");
  if (rc == 1) return;                                              // stop requested before the optimisation started (:359-361)
  // ---- write-back under the map mutex (:419-450): the observation of edge e is (kf_member[e_pose[e]], e_feat[e]), nothing is searched
  std::vector<KeyFrame*> moved;
  std::vector<MapPoint*> pts;
  {
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (int e = 0; e < E; ++e) {
      if (!erase[(size_t)e]) continue;
      KeyFrame* k = members[(size_t)kf_member[(size_t)e_pose[(size_t)e]]];
      MapPoint* p = k->GetMapPoint((size_t)e_feat[(size_t)e]);
      if (!p || p->isBad()) continue;
      k->EraseMapPointMatch((size_t)e_feat[(size_t)e]);
      p->EraseObservation(k);
    }
    for (int j = 0; j < n.n_local; ++j) {
      KeyFrame* k = members[(size_t)kf_member[(size_t)j]];
      k->SetPose(toMat(&poses[(size_t)j * 7]));
      moved.push_back(k);
    }
    for (int i = 0; i < P; ++i) {
      const std::map<int, MapPoint*>::const_iterator it = point.find(point_id[(size_t)i]);
      if (it == point.end() || !it->second || it->second->isBad()) continue;
      cv::Mat x(3, 1, CV_32F);
      for (int k = 0; k < 3; ++k) x.at<float>(k) = (float)points[(size_t)i * 3 + k];
      it->second->SetWorldPos(x);
      it->second->UpdateNormalAndDepth();
      pts.push_back(it->second);
    }
  }
  UpdateKeyFramePoses(store, moved);                                // the resident copies: ONE cms_kfstore_update_poses, ONE cms_mpstore_set
  SetMapPoints(mps, pts);
}

// ------------------------------------------------------------------------------------------------ Map-point statistics on the device
void SetMapPointStatistics(cms_mpstore* mps, const std::vector<MapPoint*>& vpMPs) {
  MpBook& m = mp_book(mps);
  std::lock_guard<std::mutex> lk(m.mu);
  std::vector<int> ids, first;
  std::set<int> named;
  for (MapPoint* p : vpMPs) {
    if (!p || p->isBad()) continue;
    const int r = row_of(m, p);
    if (r < 0 || !m.set.count(r) || !named.insert(r).second) continue;
    ids.push_back(r); first.push_back((int)p->mnFirstKFid);
  }
  if (ids.empty()) return;
  check(cms_mpstore_set_stats(mps, (int)ids.size(), ids.data(), first.data(), nullptr, nullptr), "cms_mpstore_set_stats");
}

void UpdateTrackStatistics(cms_ctx* frameCtx, cms_mpstore* mps, Frame& F, const std::vector<MapPoint*>& vpLocalMapPoints, const std::vector<uint8_t>& inView) {
  if (vpLocalMapPoints.size() != inView.size()) throw std::runtime_error("Hip::UpdateTrackStatistics: a flag per local point");
  MpBook& m = mp_book(mps);
  std::lock_guard<std::mutex> lk(m.mu);
  // IncreaseVisible() of the local points that were in view (Tracking.cpp:829) and of the frame's own points (:808: they are in view by construction)
  std::vector<int> ids;
  std::vector<uint8_t> flag;
  for (size_t i = 0; i < vpLocalMapPoints.size(); ++i) {
    MapPoint* p = vpLocalMapPoints[i];
    const int r = (p && !p->isBad()) ? row_of(m, p) : -1;
    ids.push_back(r >= 0 && m.set.count(r) ? r : -1); flag.push_back(inView[i]);
    if (ids.back() >= 0 && inView[i]) p->IncreaseVisible();
  }
  // IncreaseFound() of the frame's points the pose optimisation kept (:698)
  std::vector<int> fids((size_t)F.N, -1);
  std::vector<uint8_t> outlier((size_t)F.N, 1);
  for (int i = 0; i < F.N; ++i) {
    MapPoint* p = F.mvpMapPoints[i];
    if (!p) continue;
    const int r = row_of(m, p);
    if (r < 0 || !m.set.count(r)) continue;
    fids[(size_t)i] = r; outlier[(size_t)i] = F.mvbOutlier[i] ? 1 : 0;
    if (!F.mvbOutlier[i]) p->IncreaseFound();
  }
  const int off_l[2] = {0, (int)ids.size()}, off_f[2] = {0, F.N};
  if (!ids.empty()) check(cms_mpstore_count(mps, frameCtx, CMS_MP_VISIBLE, 1, off_l, ids.data(), flag.data(), 1), "cms_mpstore_count");
  if (F.N > 0) check(cms_mpstore_count(mps, frameCtx, CMS_MP_FOUND, 1, off_f, fids.data(), outlier.data(), 0), "cms_mpstore_count");
}

std::vector<uint8_t> MapPointCulling(cms_kfstore* store, cms_covis* covis, cms_mpstore* mps, std::list<MapPoint*>& lpRecentAddedMapPoints, KeyFrame* pCurrentKF) {
  MpBook& m = mp_book(mps);
  // held to the end: the frame thread's Hip::UpdateTrackStatistics reads m.set, and a row the device has emptied must have left it before that
  // thread can name the row again
  std::lock_guard<std::mutex> lk(m.mu);
  typedef std::list<MapPoint*>::iterator It;
  std::vector<It> at;            // the list entries that go to the device, in list order
  std::vector<int> ids, place;   // their rows, and their positions in the list
  std::set<int> named;
  int n_list = 0;
  for (It it = lpRecentAddedMapPoints.begin(); it != lpRecentAddedMapPoints.end();) {
    if ((*it)->isBad()) { it = lpRecentAddedMapPoints.erase(it); continue; }      // :187-190
    const int r = row_of(m, *it);
    // a point the table does not hold (mnId beyond it, or never set) cannot be judged here: it stays in the list, as the reference keeps every point
    // that is not bad, and gets verdict 0
    if (r >= 0 && m.set.count(r) && named.insert(r).second) { at.push_back(it); ids.push_back(r); place.push_back(n_list); }
    ++n_list; ++it;
  }
  std::vector<uint8_t> verdict((size_t)n_list, 0);
  if (ids.empty()) return verdict;
  std::vector<uint8_t> v(ids.size());
  const int off[2] = {0, (int)ids.size()};
  const int current = (int)pCurrentKF->mnId;
  check(cms_mpstore_culling(mps, covis, 1, off, ids.data(), &current, 2, 1, v.data()), "cms_mpstore_culling");
  // the pointer graph follows: SetBadFlag on the host objects of verdicts 1 and 2, the list as LocalMapping.cpp:191-205 leaves it
  StoreBook& b = book(store);
  for (size_t i = 0; i < ids.size(); ++i) {
    MapPoint* p = *at[i];
    verdict[(size_t)place[i]] = v[i];
    if (v[i] == 1 || v[i] == 2) {
      {      // the device has already written -1 where the rows named the point: the bridge's copy of the rows follows
        std::lock_guard<std::mutex> lkb(b.mu);
        const std::map<KeyFrame*, size_t> obs = p->GetObservations();
        for (std::map<KeyFrame*, size_t>::const_iterator o = obs.begin(); o != obs.end(); ++o) {
          const int s = slot_locked(b, o->first);
          if (s < 0) continue;
          std::vector<int>& row = b.dev_mp[s];
          if (o->second < row.size() && row[o->second] == ids[i]) row[o->second] = -1;
        }
      }
      p->SetBadFlag();
      m.set.erase(ids[i]); m.has_desc.erase(ids[i]); m.has_normal.erase(ids[i]);
    }
    if (v[i] == 1 || v[i] == 2 || v[i] == 3) lpRecentAddedMapPoints.erase(at[i]);      // (4, an empty row behind a live point, cannot come: m.set says the row is set)
  }
  return verdict;
}

int TrackedMapPoints(cms_covis* covis, cms_ctx* frameCtx, KeyFrame* pKF, int minObs) {
  CovisBook& c = covis_book(covis);
  int member;
  { std::lock_guard<std::mutex> lk(c.mu); member = member_of(c, pKF); }
  if (member < 0) throw std::runtime_error("Hip::TrackedMapPoints: the key frame is not a member of the last Hip::BuildCovisibility");
  int count = 0;
  check(cms_covis_tracked_map_points(covis, frameCtx, 1, &member, &minObs, &count), "cms_covis_tracked_map_points");
  return count;
}

float ComputeSceneMedianDepth(cms_kfstore* store, cms_mpstore* mps, KeyFrame* pKF, int q) {
  const int slot = slot_of(book(store), pKF);
  if (slot < 0) throw std::runtime_error("Hip::ComputeSceneMedianDepth: the key frame is not resident");
  float depth = -1.0f;
  int n = 0;
  check(cms_kfstore_scene_median_depth(store, mps, 1, &slot, q, 0, &depth, &n), "cms_kfstore_scene_median_depth");
  return depth;
}

// ------------------------------------------------------------------------------------------------ Tracking: SearchByBoW on resident key frames
namespace {
// the frame's FeatureVector (Frame::ComputeBoW) as CSR
void feat_vec_csr(const DBoW2::FeatureVector& fv, std::vector<int>& node_id, std::vector<int>& node_off, std::vector<int>& node_feat) {
  node_id.clear(); node_off.assign(1, 0); node_feat.clear();
  for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
    node_id.push_back((int)it->first);
    for (size_t q = 0; q < it->second.size(); ++q) node_feat.push_back((int)it->second[q]);
    node_off.push_back((int)node_feat.size());
  }
}
// skip flags of a key frame's features: no map point any more, or a bad one (ORBMatcher.cpp:444-450)
void bad_flags(const std::vector<MapPoint*>& v, std::vector<uint8_t>& skip) {
  skip.assign(v.size() + 1, 0);
  for (size_t i = 0; i < v.size(); ++i) skip[i] = (!v[i] || v[i]->isBad()) ? 1 : 0;
}
}  // namespace

void SearchByBoWCandidates(cms_kfstore* store, cms_ctx* frameCtx, const std::vector<KeyFrame*>& vpCandidateKFs, Frame& F,
                           std::vector<std::vector<MapPoint*> >& vvpMapPointMatches, std::vector<bool>& vbDiscarded, std::vector<int>& nmatches,
                           float nnratio, bool checkOri) {
  StoreBook& b = book(store);
  const size_t nKFs = vpCandidateKFs.size();
  vvpMapPointMatches.assign(nKFs, std::vector<MapPoint*>());
  vbDiscarded.assign(nKFs, false);
  nmatches.assign(nKFs, 0);
  std::vector<int> node_id, node_off, node_feat;
  feat_vec_csr(F.mFeatVec, node_id, node_off, node_feat);
  std::vector<cms_bow_job> jobs;
  std::vector<size_t> job_kf;
  std::vector<int> job_slot;
  std::vector<std::vector<MapPoint*> > kf_points;
  std::vector<std::vector<uint8_t> > skips;
  std::vector<int> kf_idx, nm;
  {
    // the book stays locked from the look-up to the end of the device call: the mapping thread can neither release nor refill nor update a slot
    // this search names meanwhile (ProcessNewKeyFrame, ReleaseKeyFrame and the updates of CreateNewMapPoints take the same lock)
    std::lock_guard<std::mutex> lk(b.mu);
    for (size_t i = 0; i < nKFs; ++i) {
      KeyFrame* pKF = vpCandidateKFs[i];
      const int slot = slot_locked(b, pKF);
      if (pKF->isBad() || slot < 0) { vbDiscarded[i] = true; continue; }      // Tracking.cpp:1022-1023 (and a key frame that never entered the store)
      kf_points.push_back(pKF->GetMapPointMatches());
      skips.push_back(std::vector<uint8_t>());
      bad_flags(kf_points.back(), skips.back());
      job_kf.push_back(i); job_slot.push_back(slot);
    }
    for (size_t j = 0; j < job_kf.size(); ++j) {
      cms_bow_job q;
      q.slot = job_slot[j]; q.b = 0; q.n = F.N;
      q.nnodes = (int)node_id.size(); q.node_id = node_id.data(); q.node_off = node_off.data(); q.node_feat = node_feat.data();
      q.kf_skip = skips[j].data();
      jobs.push_back(q);
    }
    kf_idx.assign(jobs.size() * (size_t)F.N + 1, -1); nm.assign(jobs.size() + 1, 0);
    if (!jobs.empty())
      check(cms_kfstore_search_by_bow(store, frameCtx, (int)jobs.size(), jobs.data(), nnratio, checkOri ? 1 : 0, kf_idx.data(), nm.data()),
            "cms_kfstore_search_by_bow");
  }
  for (size_t j = 0; j < job_kf.size(); ++j) {
    const size_t i = job_kf[j];
    std::vector<MapPoint*>& out = vvpMapPointMatches[i];
    out.assign(F.N, static_cast<MapPoint*>(NULL));
    for (int f = 0; f < F.N; ++f) {
      const int k = kf_idx[j * (size_t)F.N + f];
      if (k >= 0) out[f] = kf_points[j][k];
    }
    nmatches[i] = nm[j];
    if (nm[j] < 15) vbDiscarded[i] = true;                                 // Tracking.cpp:1027-1031
  }
}

int SearchByBoW(cms_kfstore* store, cms_ctx* frameCtx, KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches, float nnratio, bool checkOri) {
  std::vector<KeyFrame*> one(1, pKF);
  std::vector<std::vector<MapPoint*> > m;
  std::vector<bool> discarded;
  std::vector<int> n;
  if (slot_of(book(store), pKF) < 0) throw std::runtime_error("Hip::SearchByBoW: the reference key frame is not in the store");
  SearchByBoWCandidates(store, frameCtx, one, F, m, discarded, n, nnratio, checkOri);
  vpMapPointMatches = m[0].empty() ? std::vector<MapPoint*>(F.N, static_cast<MapPoint*>(NULL)) : m[0];
  return n[0];
}

// ------------------------------------------------------------------------------------------------ LoopClosing::ComputeSim3: SearchByBoW on resident key frames
void SearchByBoWLoopCandidates(cms_kfstore* store, cms_ctx* ctx, KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpCandidateKFs,
                               std::vector<std::vector<MapPoint*> >& vvpMapPointMatches, std::vector<bool>& vbDiscarded, std::vector<int>& nmatches,
                               float nnratio, bool checkOri) {
  StoreBook& b = book(store);
  const size_t nKFs = vpCandidateKFs.size();
  vvpMapPointMatches.assign(nKFs, std::vector<MapPoint*>());
  vbDiscarded.assign(nKFs, false);
  nmatches.assign(nKFs, 0);
  const std::vector<MapPoint*> vpMapPoints1 = pCurrentKF->GetMapPointMatches();
  const int n1 = (int)vpMapPoints1.size();
  std::vector<uint8_t> skip1;
  bad_flags(vpMapPoints1, skip1);
  std::vector<cms_bow_kf_job> jobs;
  std::vector<size_t> job_kf;
  std::vector<std::vector<MapPoint*> > kf_points;
  std::vector<std::vector<uint8_t> > skips;
  std::vector<int> idx2, nm;
  {
    // locked from the look-up to the end of the device call, like SearchByBoWCandidates
    std::lock_guard<std::mutex> lk(b.mu);
    const int slot1 = slot_locked(b, pCurrentKF);
    for (size_t i = 0; i < nKFs; ++i) {
      KeyFrame* pKF = vpCandidateKFs[i];
      pKF->SetNotErase();                                                    // LoopClosing.cpp:256
      const int slot2 = slot_locked(b, pKF);
      if (pKF->isBad() || slot1 < 0 || slot2 < 0) { vbDiscarded[i] = true; continue; }      // :258-262 (and a key frame that never entered the store)
      kf_points.push_back(pKF->GetMapPointMatches());
      skips.push_back(std::vector<uint8_t>());
      bad_flags(kf_points.back(), skips.back());
      cms_bow_kf_job q;
      q.slot1 = slot1; q.n1 = n1; q.slot2 = slot2; q.n2 = (int)kf_points.back().size();
      q.skip1 = skip1.data(); q.skip2 = NULL;
      jobs.push_back(q); job_kf.push_back(i);
    }
    for (size_t j = 0; j < jobs.size(); ++j) jobs[j].skip2 = skips[j].data();      // (skips no longer moves)
    idx2.assign(jobs.size() * (size_t)n1 + 1, -1); nm.assign(jobs.size() + 1, 0);
    if (!jobs.empty())
      check(cms_kfstore_search_by_bow_keyframes(store, ctx, (int)jobs.size(), jobs.data(), nnratio, checkOri ? 1 : 0, idx2.data(), nm.data()),
            "cms_kfstore_search_by_bow_keyframes");
  }
  for (size_t j = 0; j < job_kf.size(); ++j) {
    const size_t i = job_kf[j];
    std::vector<MapPoint*>& out = vvpMapPointMatches[i];
    out.assign(n1, static_cast<MapPoint*>(NULL));
    for (int f = 0; f < n1; ++f) {
      const int k = idx2[j * (size_t)n1 + f];
      if (k >= 0) out[f] = kf_points[j][k];
    }
    nmatches[i] = nm[j];
    if (nm[j] < 20) vbDiscarded[i] = true;                                   // LoopClosing.cpp:266-270
  }
}

// ------------------------------------------------------------------------------------------------ LoopClosing::ComputeSim3: SearchBySim3 on resident key frames
void SearchBySim3(cms_kfstore* store, cms_ctx* ctx, KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpKFs, std::vector<std::vector<MapPoint*> >& vvpMatches12,
                  const std::vector<float>& vs12, const std::vector<cv::Mat>& vR12, const std::vector<cv::Mat>& vt12, float th, std::vector<int>& vnFound,
                  bool zAsWritten) {
  StoreBook& b = book(store);
  const size_t nH = vpKFs.size();
  if (vvpMatches12.size() != nH || vs12.size() != nH || vR12.size() != nH || vt12.size() != nH) throw std::runtime_error("Hip::SearchBySim3: one entry per hypothesis");
  vnFound.assign(nH, 0);
  const std::vector<MapPoint*> vpMapPoints1 = pCurrentKF->GetMapPointMatches();
  const int N1 = (int)vpMapPoints1.size();
  std::vector<cms_sim3_search_job> jobs;
  std::vector<size_t> job_h;
  std::vector<std::vector<MapPoint*> > kf_points;
  std::vector<uint8_t> skip, desc;
  std::vector<float> pos, dmin, dmax;
  // one record per key point: skip <=> !pMP || vbAlreadyMatched[i] || pMP->isBad() (ORBMatcher.cpp:1410-1414, :1491-1495)
  auto records = [&](const std::vector<MapPoint*>& pts, const std::vector<bool>& matched) {
    for (size_t i = 0; i < pts.size(); ++i) {
      MapPoint* p = pts[i];
      const bool out = !p || matched[i] || p->isBad();
      skip.push_back(out ? 1 : 0);
      if (out) { pos.insert(pos.end(), 3, 0.0f); dmin.push_back(0.0f); dmax.push_back(0.0f); desc.insert(desc.end(), 32, 0); continue; }
      const cv::Mat x = p->GetWorldPos();
      for (int c = 0; c < 3; ++c) pos.push_back(x.at<float>(c));
      dmin.push_back(p->GetMinDistanceInvariance()); dmax.push_back(p->GetMaxDistanceInvariance());      // (every context of the bridge runs in distance-bounds mode 1)
      const cv::Mat d = p->GetDescriptor();
      desc.insert(desc.end(), d.data, d.data + 32);
    }
  };
  std::vector<int> idx2, nf;
  {
    // locked from the look-up to the end of the device call, like SearchByBoWLoopCandidates
    std::lock_guard<std::mutex> lk(b.mu);
    const int slot1 = slot_locked(b, pCurrentKF);
    for (size_t h = 0; h < nH; ++h) {
      KeyFrame* pKF = vpKFs[h];
      const int slot2 = slot_locked(b, pKF);
      if (slot1 < 0 || slot2 < 0) throw std::runtime_error("Hip::SearchBySim3: a key frame is not in the store");
      if ((int)vvpMatches12[h].size() != N1) throw std::runtime_error("Hip::SearchBySim3: vpMatches12 must have one entry per key point of the current key frame");
      kf_points.push_back(pKF->GetMapPointMatches());
      const std::vector<MapPoint*>& vpMapPoints2 = kf_points.back();
      const int N2 = (int)vpMapPoints2.size();
      std::vector<bool> vbAlreadyMatched1(N1, false), vbAlreadyMatched2(N2, false);      // :1387-1400
      for (int i = 0; i < N1; ++i) {
        MapPoint* pMP = vvpMatches12[h][i];
        if (pMP) {
          vbAlreadyMatched1[i] = true;
          const int i2 = pMP->GetIndexInKeyFrame(pKF);
          if (i2 >= 0 && i2 < N2) vbAlreadyMatched2[i2] = true;
        }
      }
      cms_sim3_search_job q;
      q.slot1 = slot1; q.n1 = N1; q.slot2 = slot2; q.n2 = N2; q.s12 = vs12[h];
      for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) q.R12[3 * r + c] = vR12[h].at<float>(r, c); q.t12[r] = vt12[h].at<float>(r); }
      q.off1 = (int)skip.size();
      records(vpMapPoints1, vbAlreadyMatched1);
      q.off2 = (int)skip.size();
      records(vpMapPoints2, vbAlreadyMatched2);
      jobs.push_back(q); job_h.push_back(h);
    }
    idx2.assign(jobs.size() * (size_t)N1 + 1, -1); nf.assign(jobs.size() + 1, 0);
    skip.push_back(0); pos.push_back(0.0f); dmin.push_back(0.0f); dmax.push_back(0.0f); desc.push_back(0);      // (never empty: data() stays valid)
    if (!jobs.empty())
      check(cms_kfstore_search_by_sim3(store, ctx, (int)jobs.size(), jobs.data(), (int)skip.size() - 1, skip.data(), pos.data(), dmin.data(), dmax.data(), desc.data(), th,
                                       zAsWritten ? 1 : 0, idx2.data(), nf.data()),
            "cms_kfstore_search_by_sim3");
  }
  for (size_t j = 0; j < job_h.size(); ++j) {
    const size_t h = job_h[j];
    for (int i1 = 0; i1 < N1; ++i1) {
      const int k = idx2[j * (size_t)N1 + i1];
      if (k >= 0) vvpMatches12[h][i1] = kf_points[j][k];                     // :1579
    }
    vnFound[h] = nf[j];
  }
}

// ------------------------------------------------------------------------------------------------ LoopClosing: the two projection matchers under a Sim3
namespace {
// a map point as the Scw matchers read it, or an empty record for a skipped one (never read by the device)
void push_point_or_blank(MapPoint* p, bool skipped, std::vector<float>& pos, std::vector<float>& nrm, std::vector<float>& dmin, std::vector<float>& dmax,
                         std::vector<uint8_t>& desc) {
  if (!skipped) { push_point(p, pos, nrm, dmin, dmax, desc); return; }
  pos.insert(pos.end(), 3, 0.0f); nrm.insert(nrm.end(), 3, 0.0f); dmin.push_back(0.0f); dmax.push_back(0.0f); desc.insert(desc.end(), 32, 0);
}
void scw_floats(const cv::Mat& Scw, float* out12) {
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) out12[4 * r + c] = Scw.at<float>(r, c);
}
}  // namespace

int SearchByProjection(cms_kfstore* store, cms_ctx* ctx, KeyFrame* pKF, const cv::Mat& Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th) {
  StoreBook& b = book(store);
  std::set<MapPoint*> spAlreadyFound(vpMatched.begin(), vpMatched.end());      // ORBMatcher.cpp:806-807
  spAlreadyFound.erase(static_cast<MapPoint*>(NULL));
  const int M = (int)vpPoints.size(), N = (int)vpMatched.size();
  std::vector<float> pos, nrm, dmin, dmax;
  std::vector<uint8_t> desc, skip, taken;
  for (MapPoint* p : vpPoints) {
    const bool out = p->isBad() || spAlreadyFound.count(p);                     // :817
    skip.push_back(out ? 1 : 0);
    push_point_or_blank(p, out, pos, nrm, dmin, dmax, desc);
  }
  for (MapPoint* p : vpMatched) taken.push_back(p ? 1 : 0);                     // :875 on entry
  skip.push_back(0); taken.push_back(0); pos.push_back(0.0f); nrm.push_back(0.0f); dmin.push_back(0.0f); dmax.push_back(0.0f); desc.push_back(0);      // (never empty)
  std::vector<int> match((size_t)M + 1, -1);
  int nmatches = 0;
  {
    std::lock_guard<std::mutex> lk(b.mu);                                       // from the look-up to the end of the device call, like SearchBySim3
    const int slot = slot_locked(b, pKF);
    if (slot < 0) {                                                             // not resident: the reference's own matcher
      ORBMatcher matcher(0.75, true);
      return matcher.SearchByProjection(pKF, Scw, vpPoints, vpMatched, th);
    }
    cms_sim3_proj_job q;
    q.slot = slot; q.n = N; q.set = 0;
    scw_floats(Scw, q.Scw);
    const int set_off[2] = {0, M};
    check(cms_kfstore_search_by_projection_sim3(store, ctx, 1, set_off, pos.data(), nrm.data(), dmin.data(), dmax.data(), desc.data(), 1, &q, skip.data(), taken.data(),
                                                (float)th, match.data(), &nmatches),
          "cms_kfstore_search_by_projection_sim3");
  }
  for (int i = 0; i < M; ++i) if (match[i] >= 0) vpMatched[match[i]] = vpPoints[i];      // :896
  return nmatches;
}

void SearchAndFuse(cms_kfstore* store, cms_ctx* ctx, const std::vector<std::pair<KeyFrame*, cv::Mat> >& vCorrectedPoses, const std::vector<MapPoint*>& vpLoopMapPoints,
                   Map* pMap) {
  StoreBook& b = book(store);
  const int nLP = (int)vpLoopMapPoints.size();
  // ---- one search over every resident key frame of the map, one set.  Why this equals the reference's sequential loop (LoopClosing.cpp:590-611):
  // the search result of an entry -- bestIdx -- depends only on the point's position, normal, distances and descriptor, on the key frame's key points
  // and descriptors and on Scw; none of them is changed by SearchAndFuse.  Only the skip test (:1268) and what is done with bestIdx (:1347-1358) read
  // pointer state, and both are evaluated below, live, at the key frame's turn.  A point skipped NOW is skipped then as well: isBad() never turns
  // false again, and membership of a loop point in a key frame only grows during SearchAndFuse (AddMapPoint, Replace) -- so the flags sent along
  // only spare work.
  std::vector<float> pos, nrm, dmin, dmax;
  std::vector<uint8_t> desc, skip;
  for (MapPoint* p : vpLoopMapPoints) push_point_or_blank(p, p->isBad(), pos, nrm, dmin, dmax, desc);
  pos.push_back(0.0f); nrm.push_back(0.0f); dmin.push_back(0.0f); dmax.push_back(0.0f); desc.push_back(0);      // (never empty)
  std::vector<cms_sim3_proj_job> jobs;
  std::vector<int> job_of(vCorrectedPoses.size(), -1);
  std::vector<int> best_idx, best_dist;
  {
    std::lock_guard<std::mutex> lk(b.mu);
    for (size_t k = 0; k < vCorrectedPoses.size(); ++k) {
      KeyFrame* pKF = vCorrectedPoses[k].first;
      const int slot = slot_locked(b, pKF);
      if (slot < 0) continue;
      const std::set<MapPoint*> in_kf = pKF->GetMapPoints();
      for (MapPoint* p : vpLoopMapPoints) skip.push_back((p->isBad() || in_kf.count(p)) ? 1 : 0);
      cms_sim3_proj_job q;
      q.slot = slot; q.n = (int)pKF->GetMapPointMatches().size(); q.set = 0;
      scw_floats(vCorrectedPoses[k].second, q.Scw);
      job_of[k] = (int)jobs.size();
      jobs.push_back(q);
    }
    skip.push_back(0);
    best_idx.assign(jobs.size() * (size_t)nLP + 1, -1); best_dist.assign(jobs.size() * (size_t)nLP + 1, 256);
    const int set_off[2] = {0, nLP};
    if (!jobs.empty())
      check(cms_kfstore_fuse_search_sim3(store, ctx, 1, set_off, pos.data(), nrm.data(), dmin.data(), dmax.data(), desc.data(), (int)jobs.size(), jobs.data(), skip.data(), 4.0f,
                                         best_idx.data(), best_dist.data()),
            "cms_kfstore_fuse_search_sim3");
  }
  // ---- the decisions, in the map's order and per key frame in list order, with the reference's own statements
  ORBMatcher matcher(0.8);
  for (size_t k = 0; k < vCorrectedPoses.size(); ++k) {
    KeyFrame* pKF = vCorrectedPoses[k].first;
    std::vector<MapPoint*> vpReplacePoints(vpLoopMapPoints.size(), static_cast<MapPoint*>(NULL));
    if (job_of[k] < 0) {
      matcher.Fuse(pKF, vCorrectedPoses[k].second, vpLoopMapPoints, 4, vpReplacePoints);      // not resident: the reference's own search
    } else {
      const std::set<MapPoint*> spAlreadyFound = pKF->GetMapPoints();           // ORBMatcher.cpp:1256, at this key frame's turn
      const int* bi = best_idx.data() + (size_t)job_of[k] * nLP;
      for (int i = 0; i < nLP; ++i) {
        MapPoint* pMP = vpLoopMapPoints[i];
        if (bi[i] < 0 || pMP->isBad() || spAlreadyFound.count(pMP)) continue;   // :1268
        MapPoint* pMPinKF = pKF->GetMapPoint(bi[i]);                            // :1347-1358
        if (pMPinKF) {
          if (!pMPinKF->isBad()) vpReplacePoints[i] = pMPinKF;
        } else {
          pMP->AddObservation(pKF, bi[i]);
          pKF->AddMapPoint(pMP, bi[i]);
        }
      }
    }
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                  // LoopClosing.cpp:601-610
    for (int i = 0; i < nLP; ++i) {
      MapPoint* pRep = vpReplacePoints[i];
      if (pRep) pRep->Replace(vpLoopMapPoints[i]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ Tracking::Relocalization: the guided search
int SearchByProjection(cms_kfstore* store, cms_ctx* frameCtx, Frame& CurrentFrame, KeyFrame* pKF, const std::set<MapPoint*>& sAlreadyFound, float th, int ORBdist,
                       bool checkOri) {
  // the list of ORBMatcher.cpp:268-276: the key frame's map points that are not bad and not already found, in key-point order
  const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
  std::vector<int> feat;
  std::vector<MapPoint*> pts;
  for (size_t i = 0; i < vpMPs.size(); ++i) {
    MapPoint* pMP = vpMPs[i];
    if (!pMP || pMP->isBad() || sAlreadyFound.count(pMP)) continue;
    feat.push_back((int)i); pts.push_back(pMP);
  }
  const int n = (int)pts.size();
  if (n == 0) return 0;
  std::vector<float> pos((size_t)n * 3), dmin(n), dmax(n), angle(n);
  std::vector<uint8_t> desc((size_t)n * 32);
  for (int k = 0; k < n; ++k) {
    const cv::Mat x = pts[k]->GetWorldPos();
    for (int c = 0; c < 3; ++c) pos[3 * (size_t)k + c] = x.at<float>(c);
    dmin[k] = pts[k]->GetMinDistanceInvariance();                  // the public getters: frameCtx is in cms_set_distance_bounds_mode(ctx, 1) like every context
    dmax[k] = pts[k]->GetMaxDistanceInvariance();                  // the bridge sets up
    const cv::Mat d = pts[k]->GetDescriptor();
    std::memcpy(&desc[(size_t)k * 32], d.data, 32);
    angle[k] = pKF->mvKeys[feat[k]].angle;
  }
  const int N = CurrentFrame.N;
  std::vector<int> kp_mp(N), match(n, -1);
  for (int i = 0; i < N; ++i) kp_mp[i] = CurrentFrame.mvpMapPoints[i] ? (1 << 30) : -1;      // any map point (:320): no Observations() test here
  int nm = 0;
  StoreBook& b = book(store);
  {
    // locked from the look-up to the end of the device call, like SearchByBoWCandidates
    std::lock_guard<std::mutex> lk(b.mu);
    const int slot = slot_locked(b, pKF);
    if (slot >= 0) {
      cms_kfproj_job q;
      q.slot = slot; q.b = 0; q.n = N;
      for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) q.pose12[3 * r + c] = CurrentFrame.mTcw.at<float>(r, c); q.pose12[9 + r] = CurrentFrame.mTcw.at<float>(r, 3); }
      q.nmp = n; q.kf_feat = feat.data(); q.pos = pos.data(); q.min_dist = dmin.data(); q.max_dist = dmax.data(); q.mp_desc = desc.data();
      q.kp_mp = kp_mp.data(); q.match = match.data();
      check(cms_kfstore_search_by_projection(store, frameCtx, 1, &q, th, ORBdist, checkOri ? 1 : 0, &nm), "cms_kfstore_search_by_projection");
    } else {
      // a key frame that never entered the store: its key-point angles travel with the call
      float pose12[12];
      for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) pose12[3 * r + c] = CurrentFrame.mTcw.at<float>(r, c); pose12[9 + r] = CurrentFrame.mTcw.at<float>(r, 3); }
      check(cms_search_by_projection_keyframe(frameCtx, 0, pose12, n, angle.data(), pos.data(), dmin.data(), dmax.data(), desc.data(), th, ORBdist, checkOri ? 1 : 0, N,
                                              kp_mp.data(), match.data(), &nm), "cms_search_by_projection_keyframe");
    }
  }
  for (int k = 0; k < n; ++k) if (match[k] >= 0) CurrentFrame.mvpMapPoints[match[k]] = pts[k];      // :336 (what the histogram removed is -1 again: :370)
  return nm;
}

// ---- PnPsolver (src/PnPsolver.cpp)
PnPsolver::PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches)
    : mnMatches(vpMapPointMatches.size()), mnKeys(F.mvKeys.size()), N(0), mnIterations(0), mnBestInliers(0), mRansacMinInliers(0), mRansacMaxIts(0), mRansacMinSet(4),
      mRansacEpsilon(0), mRansacTh2(5.991f) {
  std::memset(mBestTcw, 0, sizeof(mBestTcw));
  for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {      // :83-108
    MapPoint* pMP = vpMapPointMatches[i];
    if (!pMP || pMP->isBad()) continue;
    const cv::Mat Pos = pMP->GetWorldPos();
    mvP3Dw.push_back(Pos.at<float>(0)); mvP3Dw.push_back(Pos.at<float>(1)); mvP3Dw.push_back(Pos.at<float>(2));
    mvKeyPointIndices.push_back((int)i);
  }
  SetRansacParameters();
}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2) {
  N = (int)mvKeyPointIndices.size();
  mRansacMinSet = minSet; mRansacTh2 = th2;
  check(cms_pnp_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, &mRansacMinInliers, &mRansacMaxIts, &mRansacEpsilon), "cms_pnp_ransac_parameters");
  mvbBestInliers.assign((size_t)N + 1, 0);
  mvbInliers.assign((size_t)N + 1, 0);
}

void PnPsolver::FillJob(cms_pnp_job& q, int nIterations) {
  std::memset(&q, 0, sizeof(q));
  int H = 0;
  if (N >= mRansacMinInliers) H = std::max(std::max(mRansacMaxIts - mnIterations, nIterations), 0);      // the `while` of :184
  mvDraws.resize((size_t)H * 4);
  for (int i = 0; i < H; ++i)
    for (int k = 0; k < 4; ++k) mvDraws[(size_t)i * 4 + k] = DUtils::Random::RandomInt(0, N - k - 1);      // :195
  q.N = N; q.p3d = mvP3Dw.data(); q.kp_idx = mvKeyPointIndices.data(); q.b = 0; q.n = (int)mnKeys;
  q.th2 = mRansacTh2; q.min_inliers = mRansacMinInliers; q.max_its = mRansacMaxIts; q.min_set = mRansacMinSet; q.n_iterations = nIterations;
  q.n_draws = (int)mvDraws.size(); q.draws = mvDraws.data();
  q.iterations = mnIterations; q.best_inliers = mnBestInliers; std::memcpy(q.best_Tcw, mBestTcw, sizeof(mBestTcw)); q.best_mask = mvbBestInliers.data();
  q.inliers = mvbInliers.data();
}

cv::Mat PnPsolver::TakeResult(const cms_pnp_job& q, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  mnIterations = q.iterations; mnBestInliers = q.best_inliers; std::memcpy(mBestTcw, q.best_Tcw, sizeof(mBestTcw));
  bNoMore = q.no_more != 0; vbInliers.clear(); nInliers = 0;
  if (q.status == 0) return cv::Mat();
  nInliers = q.n_inliers;
  vbInliers = std::vector<bool>(mnMatches, false);      // :232-237, :250-255
  for (int i = 0; i < N; i++)
    if (mvbInliers[(size_t)i]) vbInliers[(size_t)mvKeyPointIndices[(size_t)i]] = true;
  cv::Mat Tcw = cv::Mat::eye(4, 4, CV_32F);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Tcw.at<float>(r, c) = q.Tcw[3 * r + c];
    Tcw.at<float>(r, 3) = q.Tcw[9 + r];
  }
  return Tcw;
}

cv::Mat PnPsolver::iterate(cms_pnp* pnp, cms_ctx* frameCtx, int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  cms_pnp_job q;
  FillJob(q, nIterations);
  check(cms_pnp_iterate_frames(pnp, frameCtx, 1, &q), "cms_pnp_iterate_frames");
  return TakeResult(q, bNoMore, vbInliers, nInliers);
}

cv::Mat PnPsolver::find(cms_pnp* pnp, cms_ctx* frameCtx, std::vector<bool>& vbInliers, int& nInliers) {
  bool bFlag;
  return iterate(pnp, frameCtx, mRansacMaxIts, bFlag, vbInliers, nInliers);
}

cms_pnp* CreatePnP(int maxSolvers, int maxCorrespondences, int maxHypotheses) {
  cms_pnp* pnp = nullptr;
  check(cms_pnp_create(&pnp, g_device, maxSolvers, maxCorrespondences, maxHypotheses), "cms_pnp_create");
  return pnp;
}

void IteratePnP(cms_pnp* pnp, cms_ctx* frameCtx, const std::vector<PnPsolver*>& vpSolvers, int nIterations, std::vector<cv::Mat>& vTcw, std::vector<bool>& vbNoMore,
                std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers) {
  const size_t n = vpSolvers.size();
  vTcw.assign(n, cv::Mat()); vbNoMore.assign(n, false); vvbInliers.assign(n, std::vector<bool>()); vnInliers.assign(n, 0);
  if (n == 0) return;
  std::vector<cms_pnp_job> jobs(n);
  for (size_t i = 0; i < n; ++i) vpSolvers[i]->FillJob(jobs[i], nIterations);      // the candidates' draws in the candidates' order, as the reference's loop makes them
  check(cms_pnp_iterate_frames(pnp, frameCtx, (int)n, jobs.data()), "cms_pnp_iterate_frames");
  for (size_t i = 0; i < n; ++i) {
    bool bNoMore = false;
    vTcw[i] = vpSolvers[i]->TakeResult(jobs[i], bNoMore, vvbInliers[i], vnInliers[i]);
    vbNoMore[i] = bNoMore;
  }
}

// ---- Sim3Solver (src/Sim3Solver.cpp)
Sim3Solver::Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale)
    : N(0), mN1((int)vpMatched12.size()), mnIterations(0), mnBestInliers(0), mRansacMinInliers(0), mRansacMaxIts(0), mbFixScale(bFixScale), mBestScale(0) {
  std::memset(mBestRotation, 0, sizeof(mBestRotation)); std::memset(mBestTranslation, 0, sizeof(mBestTranslation)); std::memset(mBestT12, 0, sizeof(mBestT12));
  const std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
  const cv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation(), Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
  for (int i1 = 0; i1 < mN1; i1++) {      // :66-127
    if (!vpMatched12[i1]) continue;
    MapPoint* pMP1 = vpKeyFrameMP1[i1];
    MapPoint* pMP2 = vpMatched12[i1];
    if (!pMP1) continue;
    if (pMP1->isBad() || pMP2->isBad()) continue;
    const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
    if (indexKF1 < 0 || indexKF2 < 0) continue;
    const cv::KeyPoint& kp1 = pKF1->mvKeys[indexKF1];
    const cv::KeyPoint& kp2 = pKF2->mvKeys[indexKF2];
    float u, v;
    const cv::Mat X3D1c = Rcw1 * pMP1->GetWorldPos() + tcw1;
    CamModelGeneral::GetCamera()->TransformRaysToCubemap(u, v, X3D1c.at<float>(0), X3D1c.at<float>(1), X3D1c.at<float>(2));
    if (u < 0 || v < 0) continue;
    const cv::Mat X3D2c = Rcw2 * pMP2->GetWorldPos() + tcw2;
    CamModelGeneral::GetCamera()->TransformRaysToCubemap(u, v, X3D2c.at<float>(0), X3D2c.at<float>(1), X3D2c.at<float>(2));
    if (u < 0 || v < 0) continue;
    for (int c = 0; c < 3; ++c) { mvX3Dc1.push_back(X3D1c.at<float>(c)); mvX3Dc2.push_back(X3D2c.at<float>(c)); }
    mvnMaxError1.push_back(9.210 * pKF1->mvLevelSigma2[kp1.octave]);
    mvnMaxError2.push_back(9.210 * pKF2->mvLevelSigma2[kp2.octave]);
    mvnIndices1.push_back(i1);
  }
  SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
  N = (int)mvnIndices1.size();
  mRansacMinInliers = minInliers;
  check(cms_sim3_ransac_parameters(N, probability, minInliers, maxIterations, &mRansacMaxIts), "cms_sim3_ransac_parameters");
  mnIterations = 0;
  mvbBestInliers.resize((size_t)N + 1, 0);
  mvbInliers.assign((size_t)N + 1, 0);
}

void Sim3Solver::FillJob(cms_sim3_job& q, int nIterations) {
  std::memset(&q, 0, sizeof(q));
  int H = 0;
  if (N >= mRansacMinInliers) H = std::max(std::max(mRansacMaxIts - mnIterations, nIterations), 0);      // what cms_sim3_iterate asks for
  mvDraws.resize((size_t)H * 3);
  for (int i = 0; i < H; ++i)
    for (int k = 0; k < 3; ++k) mvDraws[(size_t)i * 3 + k] = DUtils::Random::RandomInt(0, N - k - 1);      // :192
  q.N = N; q.x3dc1 = mvX3Dc1.data(); q.x3dc2 = mvX3Dc2.data(); q.max_err1 = mvnMaxError1.data(); q.max_err2 = mvnMaxError2.data();
  q.fix_scale = mbFixScale ? 1 : 0; q.min_inliers = mRansacMinInliers; q.max_its = mRansacMaxIts; q.n_iterations = nIterations;
  q.n_draws = (int)mvDraws.size(); q.draws = mvDraws.data();
  q.iterations = mnIterations; q.best_inliers = mnBestInliers; q.best_mask = mvbBestInliers.data(); q.inliers = mvbInliers.data();
  std::memcpy(q.best_R, mBestRotation, sizeof(mBestRotation)); std::memcpy(q.best_t, mBestTranslation, sizeof(mBestTranslation));
  q.best_s = mBestScale; std::memcpy(q.best_T12, mBestT12, sizeof(mBestT12));
}

cv::Mat Sim3Solver::TakeResult(const cms_sim3_job& q, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  mnIterations = q.iterations; mnBestInliers = q.best_inliers;
  std::memcpy(mBestRotation, q.best_R, sizeof(mBestRotation)); std::memcpy(mBestTranslation, q.best_t, sizeof(mBestTranslation));
  mBestScale = q.best_s; std::memcpy(mBestT12, q.best_T12, sizeof(mBestT12));
  bNoMore = q.no_more != 0; vbInliers = std::vector<bool>((size_t)mN1, false); nInliers = 0;      // :166-168
  if (q.status == 0) return cv::Mat();
  nInliers = q.n_inliers;
  for (int i = 0; i < N; i++)      // :219-221
    if (mvbInliers[(size_t)i]) vbInliers[(size_t)mvnIndices1[(size_t)i]] = true;
  cv::Mat T12 = cv::Mat::eye(4, 4, CV_32F);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) T12.at<float>(r, c) = q.T12[4 * r + c];
  return T12;
}

cv::Mat Sim3Solver::iterate(cms_sim3* sim3, cms_ctx* frameCtx, int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  cms_sim3_job q;
  FillJob(q, nIterations);
  check(cms_sim3_iterate(sim3, frameCtx, 1, &q), "cms_sim3_iterate");
  return TakeResult(q, bNoMore, vbInliers, nInliers);
}

cv::Mat Sim3Solver::find(cms_sim3* sim3, cms_ctx* frameCtx, std::vector<bool>& vbInliers12, int& nInliers) {
  bool bFlag;
  return iterate(sim3, frameCtx, mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation() {
  cv::Mat R(3, 3, CV_32F);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R.at<float>(r, c) = mBestRotation[3 * r + c];
  return R;
}
cv::Mat Sim3Solver::GetEstimatedTranslation() {
  cv::Mat t(3, 1, CV_32F);
  for (int r = 0; r < 3; ++r) t.at<float>(r) = mBestTranslation[r];
  return t;
}
float Sim3Solver::GetEstimatedScale() { return mBestScale; }

cms_sim3* CreateSim3(int maxSolvers, int maxCorrespondences, int maxHypotheses) {
  cms_sim3* sim3 = nullptr;
  check(cms_sim3_create(&sim3, g_device, maxSolvers, maxCorrespondences, maxHypotheses), "cms_sim3_create");
  return sim3;
}

void IterateSim3(cms_sim3* sim3, cms_ctx* frameCtx, const std::vector<Sim3Solver*>& vpSolvers, int nIterations, std::vector<cv::Mat>& vScm, std::vector<bool>& vbNoMore,
                 std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers) {
  const size_t n = vpSolvers.size();
  vScm.assign(n, cv::Mat()); vbNoMore.assign(n, false); vvbInliers.assign(n, std::vector<bool>()); vnInliers.assign(n, 0);
  if (n == 0) return;
  std::vector<cms_sim3_job> jobs(n);
  for (size_t i = 0; i < n; ++i) vpSolvers[i]->FillJob(jobs[i], nIterations);      // the candidates' draws in the candidates' order, as the reference's loop makes them
  check(cms_sim3_iterate(sim3, frameCtx, (int)n, jobs.data()), "cms_sim3_iterate");
  for (size_t i = 0; i < n; ++i) {
    bool bNoMore = false;
    vScm[i] = vpSolvers[i]->TakeResult(jobs[i], bNoMore, vvbInliers[i], vnInliers[i]);
    vbNoMore[i] = bNoMore;
  }
}

// ------------------------------------------------------------------------------------------------ LoopClosing::ComputeSim3: Optimizer::OptimizeSim3
cms_sim3_opt* CreateSim3Optimizer(int maxHypotheses, int maxCorrespondences) {
  cms_sim3_opt* opt = nullptr;
  check(cms_sim3_opt_create(&opt, g_device, maxHypotheses, maxCorrespondences), "cms_sim3_opt_create");
  return opt;
}

void OptimizeSim3Candidates(cms_sim3_opt* opt, cms_ctx* ctx, KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKF2, std::vector<std::vector<MapPoint*> >& vvpMatches1,
                            const std::vector<cv::Mat>& vR12, const std::vector<cv::Mat>& vt12, const std::vector<float>& vs12, float th2, bool bFixScale,
                            std::vector<Sim3Estimate>& vS12, std::vector<int>& vnInliers, int jacobian) {
  const size_t nH = vpKF2.size();
  if (vvpMatches1.size() != nH || vR12.size() != nH || vt12.size() != nH || vs12.size() != nH) throw std::runtime_error("Hip::OptimizeSim3Candidates: one entry per hypothesis");
  vS12.assign(nH, Sim3Estimate()); vnInliers.assign(nH, 0);
  if (nH == 0) return;
  struct Arrays { std::vector<float> x1, x2, k1, k2, i1, i2; std::vector<uint8_t> keep; std::vector<size_t> vnIndexEdge; };
  std::vector<Arrays> arr(nH);
  std::vector<cms_sim3_opt_job> jobs(nH);
  const cv::Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation();
  const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
  for (size_t h = 0; h < nH; ++h) {
    KeyFrame* pKF2 = vpKF2[h];
    Arrays& a = arr[h];
    const cv::Mat R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
    const int N = (int)vvpMatches1[h].size();
    for (int i = 0; i < N; ++i) {      // :941-1028
      MapPoint* pMP2 = vvpMatches1[h][i];
      if (!pMP2) continue;
      MapPoint* pMP1 = vpMapPoints1[i];
      const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
      if (!pMP1 || pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
      const cv::Mat P3D1c = R1w * pMP1->GetWorldPos() + t1w, P3D2c = R2w * pMP2->GetWorldPos() + t2w;
      const cv::KeyPoint& kp1 = pKF1->mvKeys[i];
      const cv::KeyPoint& kp2 = pKF2->mvKeys[i2];
      for (int c = 0; c < 3; ++c) { a.x1.push_back(P3D1c.at<float>(c)); a.x2.push_back(P3D2c.at<float>(c)); }
      a.k1.push_back(kp1.pt.x); a.k1.push_back(kp1.pt.y); a.k2.push_back(kp2.pt.x); a.k2.push_back(kp2.pt.y);
      a.i1.push_back(pKF1->mvInvLevelSigma2[kp1.octave]); a.i2.push_back(pKF2->mvInvLevelSigma2[kp2.octave]);
      a.vnIndexEdge.push_back((size_t)i);
    }
    const int n = (int)a.vnIndexEdge.size();
    a.keep.assign((size_t)n + 1, 1);
    a.x1.push_back(0.0f); a.x2.push_back(0.0f); a.k1.push_back(0.0f); a.k2.push_back(0.0f); a.i1.push_back(0.0f); a.i2.push_back(0.0f);      // (never empty: data() stays valid)
    cms_sim3_opt_job& q = jobs[h];
    std::memset(&q, 0, sizeof(q));
    q.N = n; q.x3dc1 = a.x1.data(); q.x3dc2 = a.x2.data(); q.kp1 = a.k1.data(); q.kp2 = a.k2.data(); q.inv_sigma2_1 = a.i1.data(); q.inv_sigma2_2 = a.i2.data();
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) q.R12[3 * r + c] = vR12[h].at<float>(r, c); q.t12[r] = vt12[h].at<float>(r); }
    q.s12 = vs12[h]; q.th2 = th2; q.fix_scale = bFixScale ? 1 : 0; q.jacobian = jacobian; q.keep = a.keep.data();
  }
  check(cms_sim3_optimize(opt, ctx, (int)nH, jobs.data()), "cms_sim3_optimize");
  for (size_t h = 0; h < nH; ++h) {
    const cms_sim3_opt_job& q = jobs[h];
    for (int k = 0; k < q.N; ++k)
      if (!arr[h].keep[(size_t)k]) vvpMatches1[h][arr[h].vnIndexEdge[(size_t)k]] = static_cast<MapPoint*>(NULL);      // :1046, :1080
    for (int c = 0; c < 4; ++c) vS12[h].q[c] = q.q12[c];
    for (int c = 0; c < 3; ++c) vS12[h].t[c] = q.t12_out[c];
    vS12[h].s = q.s12_out;
    vnInliers[h] = q.n_inliers;
  }
}

int OptimizeSim3(cms_sim3_opt* opt, cms_ctx* ctx, KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, const cv::Mat& R12, const cv::Mat& t12, float s12,
                 float th2, bool bFixScale, Sim3Estimate& S12, int jacobian) {
  std::vector<std::vector<MapPoint*> > vv(1, vpMatches1);
  std::vector<Sim3Estimate> vS;
  std::vector<int> vn;
  OptimizeSim3Candidates(opt, ctx, pKF1, std::vector<KeyFrame*>(1, pKF2), vv, std::vector<cv::Mat>(1, R12), std::vector<cv::Mat>(1, t12), std::vector<float>(1, s12), th2,
                         bFixScale, vS, vn, jacobian);
  vpMatches1 = vv[0];
  S12 = vS[0];
  return vn[0];
}

// ---- Initializer (src/Initializer.cpp)
Initializer::Initializer(const Frame& ReferenceFrame, float sigma, int iterations) : mSigma(sigma), mMaxIterations(iterations) {
  const size_t n1 = ReferenceFrame.mvKeys.size();
  mvKeys1.resize(2 * n1); mvKeyRays1.resize(3 * n1);
  for (size_t i = 0; i < n1; ++i) {
    mvKeys1[2 * i] = ReferenceFrame.mvKeys[i].pt.x; mvKeys1[2 * i + 1] = ReferenceFrame.mvKeys[i].pt.y;
    for (int c = 0; c < 3; ++c) mvKeyRays1[3 * i + c] = ReferenceFrame.mvKeyRays[i](c);
  }
}

bool Initializer::FillJob(cms_init_job& q, const Frame& CurrentFrame, const std::vector<int>& vMatches12, bool fromFrameRow) {
  std::memset(&q, 0, sizeof(q));
  const size_t n1 = mvKeys1.size() / 2, n2 = CurrentFrame.mvKeys.size();
  if (vMatches12.size() != n1) throw std::runtime_error("Hip::Initializer: vMatches12 must have one entry per key point of the reference frame");
  int N = 0;
  for (size_t i = 0; i < n1; ++i)
    if (vMatches12[i] >= 0) ++N;      // mvMatches12 (:61-73)
  if (N < 8 || mMaxIterations < 1) return false;
  mvMatches12 = vMatches12;
  if (!fromFrameRow) {
    mvKeys2.resize(2 * n2); mvKeyRays2.resize(3 * n2);
    for (size_t i = 0; i < n2; ++i) {
      mvKeys2[2 * i] = CurrentFrame.mvKeys[i].pt.x; mvKeys2[2 * i + 1] = CurrentFrame.mvKeys[i].pt.y;
      for (int c = 0; c < 3; ++c) mvKeyRays2[3 * i + c] = CurrentFrame.mvKeyRays[i](c);
    }
  }
#ifndef STUB_DUTILS_RANDOM_H      // the declarations-only stand-in of tools/check_integration_syntax.py names RandomInt alone
  DUtils::Random::SeedRandOnce(0);      // :90
#endif
  mvDraws.resize((size_t)mMaxIterations * 8);
  for (int it = 0; it < mMaxIterations; it++)
    for (int j = 0; j < 8; j++) mvDraws[(size_t)it * 8 + j] = DUtils::Random::RandomInt(0, N - j - 1);      // RandomInt(0, vAvailableIndices.size()-1), :99
  mvP3D.assign(3 * n1, 0.0f); mvbTriangulated.assign(n1, 0);
  q.n1 = (int)n1; q.n2 = (int)n2; q.keys1 = mvKeys1.data(); q.rays1 = mvKeyRays1.data();
  q.keys2 = fromFrameRow ? NULL : mvKeys2.data(); q.rays2 = fromFrameRow ? NULL : mvKeyRays2.data();
  q.matches12 = mvMatches12.data(); q.b = 0; q.sigma = mSigma; q.iterations = mMaxIterations; q.n_draws = (int)mvDraws.size(); q.draws = mvDraws.data();
  q.p3d = mvP3D.data(); q.triangulated = mvbTriangulated.data();
  return true;
}

bool Initializer::TakeResult(const cms_init_job& q, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
  R21 = cv::Mat(); t21 = cv::Mat();      // :307-308
  if (q.status != 1) return false;
  const size_t n1 = mvKeys1.size() / 2;
  vP3D.resize(n1);
  vbTriangulated = std::vector<bool>(n1, false);
  for (size_t i = 0; i < n1; ++i) {
    vP3D[i] = cv::Point3f(mvP3D[3 * i], mvP3D[3 * i + 1], mvP3D[3 * i + 2]);
    vbTriangulated[i] = mvbTriangulated[i] != 0;
  }
  R21 = cv::Mat(3, 3, CV_32F); t21 = cv::Mat(3, 1, CV_32F);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R21.at<float>(r, c) = q.R21[3 * r + c];
    t21.at<float>(r) = q.t21[r];
  }
  return true;
}

bool Initializer::InitializeWithRays(cms_init* init, cms_ctx* frameCtx, const Frame& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
                                     std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
  cms_init_job q;
  if (!FillJob(q, CurrentFrame, vMatches12, true)) { R21 = cv::Mat(); t21 = cv::Mat(); return false; }
  check(cms_init_two_view_frames(init, frameCtx, 1, &q), "cms_init_two_view_frames");
  return TakeResult(q, R21, t21, vP3D, vbTriangulated);
}

cms_init* CreateInitializer(int maxJobs, int maxMatches, int maxKeys1, int maxHypotheses) {
  cms_init* init = nullptr;
  check(cms_init_create(g_device, maxJobs, maxMatches, maxKeys1, maxHypotheses, &init), "cms_init_create");
  return init;
}

// ------------------------------------------------------------------------------------------------ ComputeBoW
cms_vocab* CreateVocabulary(const ORBVocabulary& voc, const std::string& scratchPrefix) {
  if (voc.empty()) throw std::runtime_error("Hip::CreateVocabulary: empty vocabulary");
  // one file per process and call: two processes in one directory must not share it
  static int calls = 0;
  std::ostringstream name;
  name << scratchPrefix << "." << (long)getpid() << "." << calls++ << ".txt";
  const std::string scratchFile = name.str();
  voc.saveToTextFile(scratchFile);
  std::string text;
  {
    std::ifstream f(scratchFile.c_str(), std::ios::binary);
    if (!f) throw std::runtime_error("Hip::CreateVocabulary: cannot write or read back " + scratchFile + " (pass a prefix in a writable directory)");
    std::stringstream ss;
    ss << f.rdbuf();
    text = ss.str();
  }
  std::remove(scratchFile.c_str());
  // "k L  scoring weighting", then per node "parent leaf d0 .. d31  weight" (TemplatedVocabulary.h:1429-1449); node 0 is the root
  const char* p = text.c_str();
  char* end = nullptr;
  long hdr[4];
  for (int i = 0; i < 4; ++i) { hdr[i] = std::strtol(p, &end, 10); if (end == p) throw std::runtime_error("Hip::CreateVocabulary: bad header"); p = end; }
  std::vector<int> parent(1, 0);
  std::vector<uint8_t> leaf(1, 0), desc(32, 0);
  std::vector<double> weight(1, 0.0);
  for (;;) {
    const long pid = std::strtol(p, &end, 10);
    if (end == p) break;      // the end of the text
    p = end;
    long v[33];
    for (int i = 0; i < 33; ++i) { v[i] = std::strtol(p, &end, 10); if (end == p) throw std::runtime_error("Hip::CreateVocabulary: a node line ends early"); p = end; }
    const double w = std::strtod(p, &end);
    if (end == p) throw std::runtime_error("Hip::CreateVocabulary: a node line has no weight");
    p = end;
    parent.push_back((int)pid); leaf.push_back(v[0] > 0 ? 1 : 0);
    for (int i = 0; i < 32; ++i) desc.push_back((uint8_t)v[1 + i]);
    weight.push_back(w);
  }
  cms_vocab* out = nullptr;
  check(cms_vocab_create(&out, g_device, (int)hdr[0], (int)hdr[1], (int)hdr[2], (int)hdr[3], (int)parent.size(), parent.data(), leaf.data(), desc.data(), weight.data()),
        "cms_vocab_create");
  return out;
}

namespace {
void fill_vectors(int nwords, const std::vector<int>& wid, const std::vector<double>& wval, int nnodes, const std::vector<int>& nid, const std::vector<int>& noff,
                  const std::vector<int>& nfeat, DBoW2::BowVector& bow, DBoW2::FeatureVector* fv) {
  bow.clear();
  for (int i = 0; i < nwords; ++i) bow.insert(bow.end(), std::make_pair((DBoW2::WordId)wid[i], wval[i]));
  if (!fv) return;
  fv->clear();
  for (int e = 0; e < nnodes; ++e)
    fv->insert(fv->end(), std::make_pair((DBoW2::NodeId)nid[e], std::vector<unsigned int>(nfeat.begin() + noff[e], nfeat.begin() + noff[e + 1])));
}
}  // namespace

void ComputeBoW(cms_vocab* vocab, cms_ctx* frameCtx, Frame& F) {
  if (!F.mBowVec.empty()) return;      // Frame.cpp:721
  const int row = 0, n = F.N;
  check(cms_frames_compute_bow(frameCtx, vocab, 4, 1, &row, &n), "cms_frames_compute_bow");
  const size_t cap = (size_t)std::max(n, 1);
  std::vector<int> wid(cap), nid(cap), noff(cap + 1), nfeat(cap);
  std::vector<double> wval(cap);
  int nwords = 0, nnodes = 0;
  check(cms_frames_fetch_bow(frameCtx, 0, &nwords, wid.data(), wval.data(), (int)cap, &nnodes, nid.data(), noff.data(), nfeat.data(), (int)cap, (int)cap), "cms_frames_fetch_bow");
  fill_vectors(nwords, wid, wval, nnodes, nid, noff, nfeat, F.mBowVec, &F.mFeatVec);
}

void ComputeBoW(cms_vocab* vocab, cms_kfstore* store, KeyFrame* pKF) {
  if (!pKF->mBowVec.empty() && !pKF->mFeatVec.empty()) return;      // KeyFrame.cpp:96
  StoreBook& b = book(store);
  std::lock_guard<std::mutex> lk(b.mu);      // the slot is neither released nor refilled while the call runs
  const int slot = slot_locked(b, pKF);
  if (slot < 0) throw std::runtime_error("Hip::ComputeBoW: the key frame is not in the store");
  check(cms_kfstore_compute_bow(store, vocab, 4, 1, &slot), "cms_kfstore_compute_bow");
  const size_t cap = (size_t)std::max(pKF->N, 1);
  std::vector<int> wid(cap), nid(cap), noff(cap + 1), nfeat(cap);
  std::vector<double> wval(cap);
  int nwords = 0, nnodes = 0;
  check(cms_kfstore_fetch_bow(store, slot, &nwords, wid.data(), wval.data(), (int)cap, &nnodes, nid.data(), noff.data(), nfeat.data(), (int)cap, (int)cap),
        "cms_kfstore_fetch_bow");
  fill_vectors(nwords, wid, wval, nnodes, nid, noff, nfeat, pKF->mBowVec, &pKF->mFeatVec);
}

// ------------------------------------------------------------------------------------------------ KeyFrameDatabase
namespace {

// one cms_kfdb_detect job; the covisibles of every database key frame are refreshed first (the reference reads them at the call, :156, :270)
std::vector<KeyFrame*> detect_candidates(cms_kfstore* store, cms_ctx* frameCtx, cms_kfdb_job& job) {
  StoreBook& b = book(store);
  DbBook& d = db_book(store);
  std::lock_guard<std::mutex> lk(b.mu);      // no slot of the database is refilled or released while the call runs
  std::lock_guard<std::mutex> lk2(d.mu);
  std::map<int, KeyFrame*> kf_of;
  std::vector<int> slots, neigh;
  for (KeyFrame* k : d.in_db) {
    const int s = slot_locked(b, k);
    if (s < 0) continue;
    kf_of[s] = k;
    slots.push_back(s);
    int row[10] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, n = 0;
    for (KeyFrame* c : k->GetBestCovisibilityKeyFrames(10)) {      // (one that is not in the database contributes nothing: it keeps no place)
      const int cs = slot_locked(b, c);
      if (cs >= 0 && d.in_db.count(c) && n < 10) row[n++] = cs;
    }
    neigh.insert(neigh.end(), row, row + 10);
  }
  if (slots.empty()) return std::vector<KeyFrame*>();
  check(cms_kfdb_set_covisibles(store, (int)slots.size(), slots.data(), neigh.data()), "cms_kfdb_set_covisibles");
  std::vector<int> cand(slots.size());
  int n_cand = 0;
  check(cms_kfdb_detect(store, frameCtx, 1, &job, (int)cand.size(), cand.data(), &n_cand, NULL, NULL), "cms_kfdb_detect");
  std::vector<KeyFrame*> out;
  for (int i = 0; i < n_cand; ++i) out.push_back(kf_of[cand[i]]);
  return out;
}
}  // namespace

void AddToDatabase(cms_kfstore* store, KeyFrame* pKF) {
  StoreBook& b = book(store);
  DbBook& d = db_book(store);
  std::lock_guard<std::mutex> lk(b.mu);
  const int slot = slot_locked(b, pKF);
  if (slot < 0) throw std::runtime_error("Hip::AddToDatabase: the key frame is not resident (Hip::ProcessNewKeyFrame first)");
  std::vector<int> ids;
  std::vector<double> vals;
  for (DBoW2::BowVector::const_iterator it = pKF->mBowVec.begin(); it != pKF->mBowVec.end(); ++it) { ids.push_back((int)it->first); vals.push_back(it->second); }
  check(cms_kfstore_set_bow(store, slot, (int)ids.size(), ids.data(), vals.data()), "cms_kfstore_set_bow");
  const int group = 0;
  check(cms_kfdb_add(store, 1, &slot, &group), "cms_kfdb_add");
  std::lock_guard<std::mutex> lk2(d.mu);
  d.in_db.insert(pKF);
}
void EraseFromDatabase(cms_kfstore* store, KeyFrame* pKF) {
  StoreBook& b = book(store);
  DbBook& d = db_book(store);
  std::lock_guard<std::mutex> lk(b.mu);
  std::lock_guard<std::mutex> lk2(d.mu);
  if (!d.in_db.erase(pKF)) return;      // KeyFrameDatabase::erase of a key frame that is not in it does nothing
  const int slot = slot_locked(b, pKF);
  if (slot >= 0) check(cms_kfdb_erase(store, 1, &slot), "cms_kfdb_erase");
}
void ClearDatabase(cms_kfstore* store) {
  DbBook& d = db_book(store);
  std::lock_guard<std::mutex> lk(d.mu);
  check(cms_kfdb_clear(store, -1), "cms_kfdb_clear");
  d.in_db.clear();
}
std::vector<KeyFrame*> DetectRelocalizationCandidates(cms_kfstore* store, cms_ctx* frameCtx, Frame& F) {
  cms_kfdb_job job = cms_kfdb_job();
  job.mode = CMS_KFDB_RELOC; job.group = 0; job.query = CMS_KFDB_QUERY_ROW; job.b = 0;
  return detect_candidates(store, frameCtx, job);
}
std::vector<KeyFrame*> DetectLoopCandidates(cms_kfstore* store, cms_ctx* frameCtx, KeyFrame* pKF, float minScore) {
  StoreBook& b = book(store);
  const int slot = slot_of(b, pKF);
  if (slot < 0) throw std::runtime_error("Hip::DetectLoopCandidates: the key frame is not resident (Hip::ProcessNewKeyFrame first)");
  std::vector<int> connected;
  for (KeyFrame* c : pKF->GetConnectedKeyFrames()) { const int cs = slot_of(b, c); if (cs >= 0) connected.push_back(cs); }
  cms_kfdb_job job = cms_kfdb_job();
  job.mode = CMS_KFDB_LOOP; job.group = 0; job.query = CMS_KFDB_QUERY_SLOT; job.slot = slot;
  job.min_score = minScore; job.n_connected = (int)connected.size(); job.connected = connected.empty() ? NULL : connected.data();
  return detect_candidates(store, frameCtx, job);
}
std::vector<double> LoopScore(cms_kfstore* store, KeyFrame* pKF, const std::vector<KeyFrame*>& vpOthers) {
  StoreBook& b = book(store);
  std::lock_guard<std::mutex> lk(b.mu);
  const int slot = slot_locked(b, pKF);
  if (slot < 0) throw std::runtime_error("Hip::LoopScore: the key frame is not resident");
  std::vector<int> a, o;
  for (KeyFrame* k : vpOthers) {
    const int s = slot_locked(b, k);
    if (s < 0) throw std::runtime_error("Hip::LoopScore: a key frame is not resident");
    a.push_back(slot); o.push_back(s);
  }
  std::vector<double> score(a.size());
  if (!a.empty()) check(cms_kfstore_bow_score(store, (int)a.size(), a.data(), o.data(), score.data()), "cms_kfstore_bow_score");
  return score;
}

// ---- Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:623-886) and the point loop of CorrectLoop (LoopClosing.cpp:470-500)
EssentialGraph::EssentialGraph(int device_, int max_vertices_, int max_edges_) : h(NULL), device(device_), max_vertices(0), max_edges(0), max_blocks(0) {
  Reserve(max_vertices_, max_edges_, 4LL * max_vertices_);
}
EssentialGraph::~EssentialGraph() { cms_ess_graph_destroy(h); }
void EssentialGraph::Reserve(int vertices, int edges, long long blocks) {
  if (h && vertices <= max_vertices && edges <= max_edges && blocks <= max_blocks) return;
  if (blocks > 0x7fffffffLL) throw std::runtime_error("Hip::EssentialGraph: the envelope is too large");
  cms_ess_graph_destroy(h);
  h = NULL;
  max_vertices = std::max(max_vertices, std::max(vertices, 1)); max_edges = std::max(max_edges, std::max(edges, 1)); max_blocks = std::max(max_blocks, (int)std::max(blocks, 1LL));
  check(cms_ess_graph_create(&h, device, 1, max_vertices, max_edges, max_blocks), "cms_ess_graph_create");
}

void OptimizeEssentialGraph(EssentialGraph& eg, cms_ctx* ctx, Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndEstimate& NonCorrectedSim3,
                            const KeyFrameAndEstimate& CorrectedSim3, const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections, bool bFixScale) {
  const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
  const std::vector<MapPoint*> vpMPs = pMap->GetAllMapPoints();
  const int minFeat = 100;
  // :650-686: the vertices, compacted in mnId order, bad key frames left out
  std::map<long unsigned int, KeyFrame*> byId;
  for (size_t i = 0; i < vpKFs.size(); i++)
    if (!vpKFs[i]->isBad()) byId[vpKFs[i]->mnId] = vpKFs[i];
  std::map<KeyFrame*, int> vertexOf;
  std::map<long unsigned int, int> vertexOfId;
  std::vector<KeyFrame*> vertexKF;
  std::vector<double> Scw, Snc;
  for (std::map<long unsigned int, KeyFrame*>::const_iterator it = byId.begin(); it != byId.end(); ++it) {
    KeyFrame* pKF = it->second;
    Sim3Estimate Siw;
    KeyFrameAndEstimate::const_iterator itc = CorrectedSim3.find(pKF);
    if (itc != CorrectedSim3.end()) {
      Siw = itc->second;
    } else {      // g2o::Sim3 Siw(Rcw, tcw, 1.0)
      const Eigen::Quaterniond q(Converter::toMatrix3d(pKF->GetRotation()));
      const Eigen::Matrix<double, 3, 1> t = Converter::toVector3d(pKF->GetTranslation());
      Siw.q[0] = q.x(); Siw.q[1] = q.y(); Siw.q[2] = q.z(); Siw.q[3] = q.w();
      for (int i = 0; i < 3; ++i) Siw.t[i] = t[i];
      Siw.s = 1.0;
    }
    KeyFrameAndEstimate::const_iterator itn = NonCorrectedSim3.find(pKF);
    const Sim3Estimate& Snw = itn != NonCorrectedSim3.end() ? itn->second : Siw;
    vertexOf[pKF] = (int)vertexKF.size(); vertexOfId[pKF->mnId] = (int)vertexKF.size();
    vertexKF.push_back(pKF);
    Scw.insert(Scw.end(), Siw.q, Siw.q + 4); Scw.insert(Scw.end(), Siw.t, Siw.t + 3); Scw.push_back(Siw.s);
    Snc.insert(Snc.end(), Snw.q, Snw.q + 4); Snc.insert(Snc.end(), Snw.t, Snw.t + 3); Snc.push_back(Snw.s);
  }
  if (!vertexOf.count(pLoopKF)) throw std::runtime_error("Hip::OptimizeEssentialGraph: pLoopKF has no vertex");
  std::vector<int> edges;
  std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;
  // :693-722: loop-connection edges, measured from vScw
  for (std::map<KeyFrame*, std::set<KeyFrame*> >::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
    KeyFrame* pKF = mit->first;
    const long unsigned int nIDi = pKF->mnId;
    const std::set<KeyFrame*>& spConnections = mit->second;
    for (std::set<KeyFrame*>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
      const long unsigned int nIDj = (*sit)->mnId;
      if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
      if (!vertexOf.count(pKF) || !vertexOf.count(*sit)) continue;
      edges.push_back(vertexOf[pKF]); edges.push_back(vertexOf[*sit]); edges.push_back(0);
      sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }
  // :724-825: normal edges, measured from NonCorrectedSim3 where present
  for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
    KeyFrame* pKF = vpKFs[i];
    if (!vertexOf.count(pKF)) continue;
    const int vi = vertexOf[pKF];
    KeyFrame* pParentKF = pKF->GetParent();
    if (pParentKF && vertexOf.count(pParentKF)) { edges.push_back(vi); edges.push_back(vertexOf[pParentKF]); edges.push_back(1); }      // spanning tree edge
    const std::set<KeyFrame*> sLoopEdges = pKF->GetLoopEdges();
    for (std::set<KeyFrame*>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
      KeyFrame* pLKF = *sit;
      if (pLKF->mnId < pKF->mnId && vertexOf.count(pLKF)) { edges.push_back(vi); edges.push_back(vertexOf[pLKF]); edges.push_back(1); }
    }
    const std::vector<KeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
    for (std::vector<KeyFrame*>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
      KeyFrame* pKFn = *vit;
      if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
        if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
          if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
          if (!vertexOf.count(pKFn)) continue;
          edges.push_back(vi); edges.push_back(vertexOf[pKFn]); edges.push_back(1);
        }
      }
    }
  }
  const int N = (int)vertexKF.size(), E = (int)edges.size() / 3;
  // the envelope of the unknowns (the non-fixed vertices in ascending vertex index): rows from the lowest free neighbour to the diagonal
  const int fixed = vertexOf[pLoopKF];
  std::vector<int> first((size_t)std::max(N - 1, 0));
  for (int f = 0; f < N - 1; ++f) first[(size_t)f] = f;
  for (int e = 0; e < E; ++e) {
    const int v0 = edges[3 * (size_t)e], v1 = edges[3 * (size_t)e + 1];
    if (v0 == fixed || v1 == fixed) continue;
    const int a = v0 - (v0 > fixed ? 1 : 0), b = v1 - (v1 > fixed ? 1 : 0);
    first[(size_t)std::max(a, b)] = std::min(first[(size_t)std::max(a, b)], std::min(a, b));
  }
  long long blocks = 0;
  for (int f = 0; f < N - 1; ++f) blocks += f - first[(size_t)f] + 1;
  eg.Reserve(N, E, blocks);
  std::vector<double> S_out(8 * (size_t)N);
  std::vector<float> Tiw(12 * (size_t)N);
  edges.push_back(0);
  cms_ess_graph_job q;
  std::memset(&q, 0, sizeof(q));
  q.N = N; q.Scw = Scw.data(); q.Snc = Snc.data(); q.fixed = fixed; q.E = E; q.edges = edges.data(); q.fix_scale = bFixScale ? 1 : 0;
  q.iterations = 20; q.lambda_init = 1e-16; q.S_out = S_out.data(); q.Tiw_out = Tiw.data();
  check(cms_essential_graph_optimize(eg.h, ctx, 1, &q), "cms_essential_graph_optimize");
  // :854-885: the map points through their reference key frames
  std::vector<float> pos(3 * vpMPs.size() + 3), pos_out(3 * vpMPs.size() + 3);
  std::vector<int> ref(vpMPs.size() + 1, -1);
  for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
    MapPoint* pMP = vpMPs[i];
    if (pMP->isBad()) continue;
    const long unsigned int nIDr = pMP->mnCorrectedByKF == pCurKF->mnId ? pMP->mnCorrectedReference : pMP->GetReferenceKeyFrame()->mnId;
    std::map<long unsigned int, int>::const_iterator it = vertexOfId.find(nIDr);
    if (it == vertexOfId.end()) continue;
    const cv::Mat P3Dw = pMP->GetWorldPos();
    for (int c = 0; c < 3; ++c) pos[3 * i + c] = P3Dw.at<float>(c);
    ref[i] = it->second;
  }
  check(cms_sim3_correct_points(ctx, (int)vpMPs.size(), pos.data(), ref.data(), N, Scw.data(), S_out.data(), pos_out.data()), "cms_sim3_correct_points");
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
  for (int v = 0; v < N; ++v) {      // :833-852
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) T.at<float>(r, c) = Tiw[12 * (size_t)v + 4 * r + c];
    vertexKF[(size_t)v]->SetPose(T);
  }
  for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
    if (ref[i] < 0) continue;
    cv::Mat P(3, 1, CV_32F);
    for (int c = 0; c < 3; ++c) P.at<float>(c) = pos_out[3 * i + c];
    vpMPs[i]->SetWorldPos(P);
    vpMPs[i]->UpdateNormalAndDepth();
  }
}

void CorrectLoopPoints(cms_ctx* ctx, const KeyFrameAndEstimate& CorrectedSim3, const KeyFrameAndEstimate& NonCorrectedSim3, KeyFrame* pCurKF) {
  std::vector<double> S_old, S_new;
  std::vector<MapPoint*> pts;
  std::vector<KeyFrame*> owner;
  std::vector<float> pos;
  std::vector<int> ref;
  std::set<MapPoint*> taken;      // a point seen from two key frames is corrected by the first, as mnCorrectedByKF makes the reference do
  int k = 0;
  for (KeyFrameAndEstimate::const_iterator mit = CorrectedSim3.begin(), mend = CorrectedSim3.end(); mit != mend; mit++, k++) {
    KeyFrame* pKFi = mit->first;
    const Sim3Estimate& corrected = mit->second;
    KeyFrameAndEstimate::const_iterator itn = NonCorrectedSim3.find(pKFi);
    if (itn == NonCorrectedSim3.end()) throw std::runtime_error("Hip::CorrectLoopPoints: a corrected key frame without its non-corrected pose");
    const Sim3Estimate& plain = itn->second;
    S_new.insert(S_new.end(), corrected.q, corrected.q + 4); S_new.insert(S_new.end(), corrected.t, corrected.t + 3); S_new.push_back(corrected.s);
    S_old.insert(S_old.end(), plain.q, plain.q + 4); S_old.insert(S_old.end(), plain.t, plain.t + 3); S_old.push_back(plain.s);
    const std::vector<MapPoint*> vpMPsi = pKFi->GetMapPointMatches();
    for (size_t iMP = 0, endMPi = vpMPsi.size(); iMP < endMPi; iMP++) {
      MapPoint* pMPi = vpMPsi[iMP];
      if (!pMPi) continue;
      if (pMPi->isBad()) continue;
      if (pMPi->mnCorrectedByKF == pCurKF->mnId || taken.count(pMPi)) continue;
      taken.insert(pMPi);
      const cv::Mat P3Dw = pMPi->GetWorldPos();
      for (int c = 0; c < 3; ++c) pos.push_back(P3Dw.at<float>(c));
      ref.push_back(k); pts.push_back(pMPi); owner.push_back(pKFi);
    }
  }
  const int n = (int)pts.size();
  std::vector<float> out(3 * (size_t)n + 3);
  pos.push_back(0.0f); ref.push_back(-1);
  check(cms_sim3_correct_points(ctx, n, pos.data(), ref.data(), k, S_old.data(), S_new.data(), out.data()), "cms_sim3_correct_points");
  for (int i = 0; i < n; ++i) {
    cv::Mat P(3, 1, CV_32F);
    for (int c = 0; c < 3; ++c) P.at<float>(c) = out[3 * (size_t)i + c];
    pts[(size_t)i]->SetWorldPos(P);
    pts[(size_t)i]->mnCorrectedByKF = pCurKF->mnId;
    pts[(size_t)i]->mnCorrectedReference = owner[(size_t)i]->mnId;
    pts[(size_t)i]->UpdateNormalAndDepth();
  }
}

}  // namespace Hip
