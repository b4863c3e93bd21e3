// cubemap_hot_path.cpp -- host-side mirror of the reference interfaces over the C-ABI (see cubemap_hot_path.h).
#include "cubemap_hot_path.h"
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <fstream>
#include <iomanip>
#include <stdexcept>
#include <map>
#include "../csrc/cms_vocab_core.h"
#include "../csrc/cms_kfdb_core.h"
#include "../csrc/cms_covis_core.h"
#include "../csrc/cms_mappoint_core.h"
#include "../csrc/cms_mpstats_core.h"
#include "../csrc/cms_ba_window_core.h"
#include "../csrc/cms_ess_graph_core.h"      // CmsS3 and Sim3(R, t, s) for vScw
#include "../csrc/cms_ess_graph_job_check.h" // the envelope count for the handle
#include "../csrc/cms_sim3_core.h"      // the gemm rule (cms_sim3_row) and TransformRaysToCubemap for the constructor's filter

namespace CubemapSLAM {

// ------------------------------------------------------------------------------------------------ camera singleton
CamModelGeneral* CamModelGeneral::GetCamera() {
  static CamModelGeneral* cam = new CamModelGeneral();   // CamModelGeneral.cpp:31-38
  return cam;
}
void CamModelGeneral::SetCamParams(const double cdeu0v0[5], const std::vector<double>& poly, const std::vector<double>& invpoly,
                                   double Iw, double Ih, double, double, double, double, double width, double height, double camFov) {
  std::memset(&cam_, 0, sizeof(cam_));
  cam_.c = cdeu0v0[0]; cam_.d = cdeu0v0[1]; cam_.e = cdeu0v0[2]; cam_.u0 = cdeu0v0[3]; cam_.v0 = cdeu0v0[4];
  for (size_t i = 0; i < invpoly.size() && i < 12; ++i) cam_.invpol[i] = invpoly[i];
  for (size_t i = 0; i < poly.size() && i < 5; ++i) cam_.pol[i] = poly[i];
  cam_.Iw = (int)Iw; cam_.Ih = (int)Ih;
  if ((int)width != (int)height) throw std::runtime_error("CubeFace.w must equal CubeFace.h");
  cam_.face = (int)width;
  cam_.fov_deg = camFov;
  const float fov = (float)camFov;
  cosFovTh_ = cosf(fov / 2 * (3.1415926535897932384626f / 180));   // CamModelGeneral.h:224-229
  configured_ = true;
}
CamModelGeneral::eFace CamModelGeneral::FaceInCubemap(const cv::Point2f& pixel) const {
  const double i = pixel.x / (float)cam_.face, j = pixel.y / (float)cam_.face;
  if (i >= 0 && i < 1 && j >= 1 && j < 2) return LEFT_FACE;
  if (i >= 1 && i < 2 && j >= 0 && j < 1) return UPPER_FACE;
  if (i >= 1 && i < 2 && j >= 1 && j < 2) return FRONT_FACE;
  if (i >= 1 && i < 2 && j >= 2 && j < 3) return LOWER_FACE;
  if (i >= 2 && i < 3 && j >= 1 && j < 2) return RIGHT_FACE;
  return UNKNOWN_FACE;
}
void CamModelGeneral::GetPosInFace(double& u, double& v, double uCubemap, double vCubemap) const {
  const int i = (int)std::floor(uCubemap / cam_.face), j = (int)std::floor(vCubemap / cam_.face);
  u = uCubemap - i * cam_.face; v = vCubemap - j * cam_.face;
}

// ------------------------------------------------------------------------------------------------ shared device context
static std::mutex g_ctx_mutex;
static cms_ctx* g_ctx = nullptr;
static const int kSharedDevice = 0;      // the device of the shared context (and of what works with it: ORBVocabulary's device handle)
static cms_orb_params g_ctx_orb{};
static cms_kfstore* g_bow_kf_store = nullptr;      // ORBMatcher::SearchByBoW(pKF1, pKF2, ...) and SearchBySim3: two slots on the shared context, made by the first call
static cms_camera g_ctx_cam{};      // the camera the shared context was built for (SetCamParams zero-fills the record first: comparable byte for byte)
cms_ctx* SharedContext(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST) {
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  cms_orb_params orb{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST};
  if (!CamModelGeneral::GetCamera()->configured()) throw std::runtime_error("CamModelGeneral::SetCamParams was not called");
  // the context belongs to (camera, extractor parameters): a process that configures the camera singleton again (another sequence, another face
  // size) gets a new one -- until round 6 only the extractor parameters were compared, and the mirror kept searching with the OLD camera's LUT and grid
  if (g_ctx && std::memcmp(&orb, &g_ctx_orb, sizeof(orb)) == 0 && std::memcmp(&g_ctx_cam, &CamModelGeneral::GetCamera()->params(), sizeof(cms_camera)) == 0) return g_ctx;
  if (g_bow_kf_store) { cms_kfstore_destroy(g_bow_kf_store); g_bow_kf_store = nullptr; }      // (it lives on the context that goes)
  if (g_ctx) { cms_ctx_destroy(g_ctx); g_ctx = nullptr; }
  const int rc = cms_ctx_create(&g_ctx, kSharedDevice, &CamModelGeneral::GetCamera()->params(), &orb, 1);
  if (rc != CMS_OK) throw std::runtime_error(std::string("cms_ctx_create: ") + cms_last_error());
  g_ctx_orb = orb; g_ctx_cam = CamModelGeneral::GetCamera()->params();
  return g_ctx;
}

// ------------------------------------------------------------------------------------------------ remap
void System::CreateUndistortRectifyMap() { SharedContext(2000, 1.2f, 8, 20, 7); }
void System::CvtFisheyeToCubeMap_reverseQuery_withInterpolation(cv::Mat& cubemapImg, const cv::Mat& fisheyeImg, int interpolation,
                                                                int borderType, const cv::Scalar&) {
  if (interpolation != cv::INTER_LINEAR || borderType != cv::BORDER_CONSTANT)
    throw std::runtime_error("only INTER_LINEAR / BORDER_CONSTANT(0) -- the mode the reference's examples use (cubemap_lafida.cpp:143)");
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  if (!g_ctx) throw std::runtime_error("CreateUndistortRectifyMap was not called");
  if (cms_remap(g_ctx, fisheyeImg.data, (int)fisheyeImg.step, cubemapImg.data, (int)cubemapImg.step) != CMS_OK)
    throw std::runtime_error(std::string("cms_remap: ") + cms_last_error());
}

// ------------------------------------------------------------------------------------------------ extractor
ORBextractor::ORBextractor(int _nfeatures, float _scaleFactor, int _nlevels, int _iniThFAST, int _minThFAST)
    : nfeatures(_nfeatures), scaleFactor(_scaleFactor), nlevels(_nlevels), iniThFAST(_iniThFAST), minThFAST(_minThFAST) {
  ctx_ = SharedContext(nfeatures, (float)scaleFactor, nlevels, iniThFAST, minThFAST);
  cms_geometry g;
  cms_ctx_geometry(ctx_, &g);
  for (int l = 0; l < nlevels; ++l) {
    mvScaleFactor.push_back(g.scale[l]); mvInvScaleFactor.push_back(g.inv_scale[l]);
    mvLevelSigma2.push_back(g.sigma2[l]); mvInvLevelSigma2.push_back(g.inv_sigma2[l]);
  }
}
void ORBextractor::operator()(cv::InputArray image, cv::InputArray mask, std::vector<cv::KeyPoint>& keypoints,
                              cv::OutputArray descriptors) {
  if (image.empty()) return;                                        // ORBExtractor.cpp:841
  assert(image.type() == cv::CV_8UC1);                              // :845
  assert(mask.type() == cv::CV_8UC1 && !mask.empty());              // :848
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  cms_geometry g;
  cms_ctx_geometry(ctx_, &g);
  if (image.cols != g.W || image.rows != g.W || mask.cols != g.W || mask.rows != g.W)
    throw std::runtime_error("ORBextractor: image / mask must be the 3F x 3F cubemap canvas");
  if (mask.data != last_mask_) {   // the mask is constant per sequence: upload once per distinct buffer
    if (cms_set_mask(ctx_, mask.data, (int)mask.step) != CMS_OK) throw std::runtime_error(cms_last_error());
    last_mask_ = mask.data;
  }
  std::vector<cms_keypoint> kps(g.kp_cap);
  std::vector<uint8_t> desc((size_t)g.kp_cap * 32);
  int n = 0;
  if (cms_extract(ctx_, image.data, (int)image.step, kps.data(), desc.data(), g.kp_cap, &n) != CMS_OK)
    throw std::runtime_error(std::string("cms_extract: ") + cms_last_error());
  keypoints.clear();
  keypoints.reserve(n);
  for (int i = 0; i < n; ++i) {
    cv::KeyPoint kp;
    kp.pt = cv::Point2f(kps[i].x, kps[i].y); kp.size = kps[i].size; kp.angle = kps[i].angle; kp.response = kps[i].response;
    kp.octave = kps[i].octave;
    keypoints.push_back(kp);
  }
  if (mbKeepImagePyramid) {                                         // ORBExtractor.h:89: mvImagePyramid of the last call
    mvImagePyramid.resize(g.nlevels); mvMaskPyramid.resize(g.nlevels);
    for (int l = 0; l < g.nlevels; ++l) {
      mvImagePyramid[l].create(g.level_h[l], g.level_w[l], cv::CV_8U);
      if (cms_debug_level(ctx_, 0, l, mvImagePyramid[l].data, (int)mvImagePyramid[l].step) != CMS_OK) throw std::runtime_error(cms_last_error());
    }
  }
  if (n == 0) { descriptors.release(); return; }                    // ORBExtractor.cpp:863-864
  descriptors.create(n, 32, cv::CV_8U);
  for (int i = 0; i < n; ++i) std::memcpy(descriptors.ptr<uint8_t>(i), &desc[(size_t)i * 32], 32);
}

// ------------------------------------------------------------------------------------------------ matcher
int ORBMatcher::DescriptorDistance(const cv::Mat& a, const cv::Mat& b) {
  const uint32_t* pa = a.ptr<uint32_t>();
  const uint32_t* pb = b.ptr<uint32_t>();
  int dist = 0;
  for (int i = 0; i < 8; ++i) dist += __builtin_popcount(pa[i] ^ pb[i]);
  return dist;
}

namespace {
struct KfPack {                                            // flat buffers behind one cms_keyframe
  std::vector<cms_keypoint> kps; std::vector<uint8_t> desc; std::vector<float> rays; std::vector<int> mp, node_id, node_off, node_feat;
};
void pose15_from_Tcw(const cv::Mat& Tcw, float* R, float* t, float* Ow) {
  // KeyFrame::SetPose (KeyFrame.cpp): Rcw, tcw, Ow = -Rcw.t()*tcw (transposed operand: double accumulation, one rounding)
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) R[3 * r + c] = Tcw.at<float>(r, c); t[r] = Tcw.at<float>(r, 3); }
  for (int r = 0; r < 3; ++r) {
    double s = 0;
    for (int k = 0; k < 3; ++k) s += (double)Tcw.at<float>(k, r) * (double)Tcw.at<float>(k, 3);
    Ow[r] = (float)(-1.0 * s);
  }
}
cms_keyframe pack_keyframe(const KeyFrameView& kf, KfPack& b) {
  const int N = (int)kf.mvKeys.size();
  b.kps.resize(N + 1); b.desc.resize(32 * (size_t)N + 32); b.rays.resize(3 * (size_t)N + 3); b.mp.resize(N + 1);
  for (int i = 0; i < N; ++i) {
    const cv::KeyPoint& k = kf.mvKeys[i];
    b.kps[i].x = k.pt.x; b.kps[i].y = k.pt.y; b.kps[i].size = k.size; b.kps[i].angle = k.angle; b.kps[i].response = k.response; b.kps[i].octave = k.octave;
    std::memcpy(&b.desc[32 * (size_t)i], kf.mDescriptors.ptr<uint8_t>(i), 32);
    for (int c = 0; c < 3; ++c) b.rays[3 * (size_t)i + c] = kf.mvKeyRays[i].v[c];
    b.mp[i] = kf.mvpMapPoints[i] >= 0 ? 1 : -1;
  }
  b.node_off.assign(1, 0);
  for (const auto& e : kf.mFeatVec) {
    b.node_id.push_back((int)e.first);
    for (unsigned f : e.second) b.node_feat.push_back((int)f);
    b.node_off.push_back((int)b.node_feat.size());
  }
  if (b.node_feat.empty()) b.node_feat.push_back(0);
  if (b.node_id.empty()) b.node_id.push_back(0);
  cms_keyframe k{};
  k.n = N; k.kps = b.kps.data(); k.desc = b.desc.data(); k.rays = b.rays.data(); k.mp = b.mp.data();
  pose15_from_Tcw(kf.Tcw, k.Rcw, k.tcw, k.Ow);
  k.nnodes = (int)kf.mFeatVec.size(); k.node_id = b.node_id.data(); k.node_off = b.node_off.data(); k.node_feat = b.node_feat.data();
  k.median_depth = kf.medianDepth;
  return k;
}
}  // namespace

std::vector<NewMapPoint> LocalMapping::CreateNewMapPoints(const KeyFrameView& cur, const std::vector<const KeyFrameView*>& neigh) {
  std::vector<NewMapPoint> out;
  if (neigh.empty() || cur.mvKeys.empty()) return out;
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  KfPack pc;
  std::vector<KfPack> pn(neigh.size());
  const cms_keyframe kc = pack_keyframe(cur, pc);
  std::vector<cms_keyframe> kn(neigh.size());
  for (size_t i = 0; i < neigh.size(); ++i) kn[i] = pack_keyframe(*neigh[i], pn[i]);
  const int off[2] = {0, (int)neigh.size()};
  const int cap = (int)cur.mvKeys.size();
  std::vector<int> on(cap), o1(cap), o2(cap);
  std::vector<float> ox(3 * (size_t)cap);
  int n_new = 0;
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (cms_create_new_map_points(ctx, 1, &kc, off, kn.data(), 0 /* ORBMatcher matcher(0.6,false) */, cap, &n_new, on.data(), o1.data(), o2.data(),
                                  ox.data()) != CMS_OK)
      throw std::runtime_error(std::string("cms_create_new_map_points: ") + cms_last_error());
  }
  out.resize(n_new);
  for (int k = 0; k < n_new; ++k) {
    out[k].neighbour = on[k]; out[k].idx1 = o1[k]; out[k].idx2 = o2[k];
    for (int c = 0; c < 3; ++c) out[k].x3D.v[c] = ox[3 * (size_t)k + c];
  }
  return out;
}

int ORBMatcher::Fuse(KeyFrameView& kf, const std::vector<MapPointView>& mps, const std::vector<uint8_t>& skip, float th, std::vector<int>& fused) {
  const int N = (int)kf.mvKeys.size(), M = (int)mps.size();
  fused.assign(M, -1);
  if (M == 0 || N == 0) return 0;
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  float pose15[15];
  pose15_from_Tcw(kf.Tcw, pose15, pose15 + 9, pose15 + 12);
  std::vector<float> pos(3 * (size_t)M), nrm(3 * (size_t)M), dmin(M), dmax(M);
  std::vector<uint8_t> desc(32 * (size_t)M);
  for (int i = 0; i < M; ++i) {
    for (int k = 0; k < 3; ++k) { pos[3 * (size_t)i + k] = mps[i].mWorldPos.at<float>(k, 0); nrm[3 * (size_t)i + k] = mps[i].mNormalVector.at<float>(k, 0); }
    dmin[i] = mps[i].mfMinDistance; dmax[i] = mps[i].mfMaxDistance;
    std::memcpy(&desc[32 * (size_t)i], mps[i].mDescriptor.ptr<uint8_t>(0), 32);
  }
  std::vector<cms_keypoint> kps(N);
  std::vector<uint8_t> tdesc(32 * (size_t)N);
  for (int j = 0; j < N; ++j) {
    const cv::KeyPoint& k = kf.mvKeys[j];
    kps[j].x = k.pt.x; kps[j].y = k.pt.y; kps[j].size = k.size; kps[j].angle = k.angle; kps[j].response = k.response; kps[j].octave = k.octave;
    std::memcpy(&tdesc[32 * (size_t)j], kf.mDescriptors.ptr<uint8_t>(j), 32);
  }
  std::vector<int> bi(M), bd(M);
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    int rc = cms_area_set_keypoints(ctx, 0, N, kps.data());
    if (rc == CMS_OK) rc = cms_area_set_descriptors(ctx, 0, N, tdesc.data());
    if (rc == CMS_OK) rc = cms_area_grid(ctx, 1);
    if (rc == CMS_OK) rc = cms_fuse_search(ctx, 0, pose15, M, skip.empty() ? nullptr : skip.data(), pos.data(), nrm.data(), dmin.data(), dmax.data(), desc.data(),
                                           th, bi.data(), bd.data());
    if (rc != CMS_OK) throw std::runtime_error(std::string("cms_fuse_search: ") + cms_last_error());
  }
  // ORBMatcher.cpp:1216-1241 in list order.  A key point that already holds a point means Replace (which of the two survives is the
  // caller's Observations() comparison); a free one receives the observation -- and then holds a point for the rest of the list.
  int nFused = 0;
  for (int i = 0; i < M; ++i) {
    if (bi[i] < 0) continue;
    fused[i] = bi[i];
    if (kf.mvpMapPoints[bi[i]] < 0) kf.mvpMapPoints[bi[i]] = mps[i].mnId;
    ++nFused;
  }
  return nFused;
}

int Tracking::SearchLocalPoints(FrameView& F, std::vector<MapPointView>& mps, float th, float nnratio, float viewingCosLimit) {
  const int N = (int)F.mvKeys.size(), M = (int)mps.size();
  if (M == 0) return 0;
  if (F.mTcw.rows != 4 || F.mTcw.cols != 4 || F.mTcw.type() != cv::CV_32F) throw std::runtime_error("SearchLocalPoints: mTcw must be 4x4 CV_32F");
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  // Frame::UpdatePoseMatrices (Frame.cpp:189-195): mRcw, mtcw and mOw = -mRcw.t()*mtcw (cv::gemm with a transposed operand:
  // double accumulation, one rounding to float)
  float pose15[15];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) pose15[3 * r + c] = F.mTcw.at<float>(r, c);
    pose15[9 + r] = F.mTcw.at<float>(r, 3);
  }
  for (int r = 0; r < 3; ++r) {
    double s = 0;
    for (int k = 0; k < 3; ++k) s += (double)F.mTcw.at<float>(k, r) * (double)F.mTcw.at<float>(k, 3);
    pose15[12 + r] = (float)(-1.0 * s);
  }
  std::vector<float> pos(3 * (size_t)M), nrm(3 * (size_t)M), dmin(M), dmax(M);
  std::vector<uint8_t> desc(32 * (size_t)M);
  for (int i = 0; i < M; ++i) {
    for (int k = 0; k < 3; ++k) { pos[3 * (size_t)i + k] = mps[i].mWorldPos.at<float>(k, 0); nrm[3 * (size_t)i + k] = mps[i].mNormalVector.at<float>(k, 0); }
    dmin[i] = mps[i].mfMinDistance; dmax[i] = mps[i].mfMaxDistance;
    std::memcpy(&desc[32 * (size_t)i], mps[i].mDescriptor.ptr<uint8_t>(0), 32);
  }
  std::vector<cms_keypoint> kps(N);
  std::vector<uint8_t> tdesc(32 * (size_t)N);
  std::vector<int> kp_mp(N, -1);
  for (int j = 0; j < N; ++j) {
    const cv::KeyPoint& k = F.mvKeys[j];
    kps[j].x = k.pt.x; kps[j].y = k.pt.y; kps[j].size = k.size; kps[j].angle = k.angle; kps[j].response = k.response; kps[j].octave = k.octave;
    std::memcpy(&tdesc[32 * (size_t)j], F.mDescriptors.ptr<uint8_t>(j), 32);
    if (F.mvpMapPoints[j] >= 0) kp_mp[j] = 0x40000000;           // holds a map point already (ORBMatcher.cpp:91-93)
  }
  std::vector<uint8_t> vis(M);
  std::vector<float> px(M), py(M), vc(M);
  std::vector<int> lvl(M), match(M);
  int nm = 0;
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    int rc = cms_area_set_keypoints(ctx, 0, N, kps.data());
    if (rc == CMS_OK) rc = cms_area_set_descriptors(ctx, 0, N, tdesc.data());
    if (rc == CMS_OK) rc = cms_area_grid(ctx, 1);
    if (rc == CMS_OK) rc = cms_search_local_points(ctx, 0, pose15, M, pos.data(), nrm.data(), dmin.data(), dmax.data(), desc.data(), viewingCosLimit, th,
                                                   nnratio, ORBMatcher::TH_HIGH, N, kp_mp.data(), vis.data(), px.data(), py.data(), lvl.data(), vc.data(),
                                                   match.data(), &nm, nullptr);
    if (rc != CMS_OK) throw std::runtime_error(std::string("cms_search_local_points: ") + cms_last_error());
  }
  for (int i = 0; i < M; ++i) {
    mps[i].mbTrackInView = vis[i] != 0; mps[i].mTrackProjX = px[i]; mps[i].mTrackProjY = py[i];
    mps[i].mnTrackScaleLevel = lvl[i]; mps[i].mTrackViewCos = vc[i];
    if (match[i] >= 0) F.mvpMapPoints[match[i]] = mps[i].mnId;
  }
  return nm;
}

int ORBMatcher::SearchByProjection(FrameView& F, std::vector<MapPointView>& vpMapPoints, float th) {
  // the reference walks vpMapPoints and skips !mbTrackInView (ORBMatcher.cpp:58-59): the marked ones go to the device as one list, in order
  std::vector<MapPointView> marked;
  std::vector<size_t> src;
  for (size_t i = 0; i < vpMapPoints.size(); ++i)
    if (vpMapPoints[i].mbTrackInView) { marked.push_back(vpMapPoints[i]); src.push_back(i); }
  if (marked.empty()) return 0;
  // viewing-cosine limit below any cosine: the caller's isInFrustum applied its own; every other test of isInFrustum repeats with the same result
  const int n = Tracking::SearchLocalPoints(F, marked, th, mfNNratio, -2.0f);
  for (size_t k = 0; k < src.size(); ++k) {
    MapPointView& d = vpMapPoints[src[k]];
    d.mTrackProjX = marked[k].mTrackProjX; d.mTrackProjY = marked[k].mTrackProjY; d.mnTrackScaleLevel = marked[k].mnTrackScaleLevel; d.mTrackViewCos = marked[k].mTrackViewCos;
  }
  return n;
}

int ORBMatcher::SearchForInitialization(FrameView& F1, FrameView& F2, std::vector<cv::Point2f>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize) {
  const int N1 = (int)F1.mvKeys.size(), N2 = (int)F2.mvKeys.size();
  vnMatches12.assign(N1, -1);
  if (N1 == 0 || N2 == 0) return 0;
  if ((int)vbPrevMatched.size() != N1) throw std::runtime_error("SearchForInitialization: vbPrevMatched must have one entry per key point of F1");
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  auto pack = [](const FrameView& f, std::vector<cms_keypoint>& k, std::vector<uint8_t>& d) {
    const int n = (int)f.mvKeys.size();
    k.resize(n); d.resize(32 * (size_t)n);
    for (int j = 0; j < n; ++j) {
      const cv::KeyPoint& q = f.mvKeys[j];
      k[j].x = q.pt.x; k[j].y = q.pt.y; k[j].size = q.size; k[j].angle = q.angle; k[j].response = q.response; k[j].octave = q.octave;
      std::memcpy(&d[32 * (size_t)j], f.mDescriptors.ptr<uint8_t>(j), 32);
    }
  };
  std::vector<cms_keypoint> k1, k2;
  std::vector<uint8_t> d1, d2;
  pack(F1, k1, d1); pack(F2, k2, d2);
  std::vector<float> prev(2 * (size_t)N1);
  for (int i = 0; i < N1; ++i) { prev[2 * (size_t)i] = vbPrevMatched[i].x; prev[2 * (size_t)i + 1] = vbPrevMatched[i].y; }
  int nm = 0;
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    int rc = cms_area_set_keypoints(ctx, 0, N2, k2.data());
    if (rc == CMS_OK) rc = cms_area_set_descriptors(ctx, 0, N2, d2.data());
    if (rc == CMS_OK) rc = cms_area_grid(ctx, 1);
    if (rc == CMS_OK) rc = cms_search_for_initialization(ctx, 0, N1, k1.data(), d1.data(), prev.data(), windowSize, mfNNratio, mbCheckOrientation ? 1 : 0,
                                                         vnMatches12.data(), &nm);
    if (rc != CMS_OK) throw std::runtime_error(std::string("cms_search_for_initialization: ") + cms_last_error());
  }
  for (int i = 0; i < N1; ++i) vbPrevMatched[i] = cv::Point2f(prev[2 * (size_t)i], prev[2 * (size_t)i + 1]);
  return nm;
}

int ORBMatcher::SearchForTriangulation(const KeyFrameView& pKF1, const KeyFrameView& pKF2, const cv::Mat& E12, std::vector<std::pair<size_t, size_t>>& vMatchedPairs) {
  vMatchedPairs.clear();
  if (pKF1.mvKeys.empty() || pKF2.mvKeys.empty()) return 0;
  if (E12.rows != 3 || E12.cols != 3 || E12.type() != cv::CV_32F) throw std::runtime_error("SearchForTriangulation: E12 must be 3x3 CV_32F");
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  KfPack p1, p2;
  const cms_keyframe k1 = pack_keyframe(pKF1, p1), k2 = pack_keyframe(pKF2, p2);
  float e[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) e[3 * r + c] = E12.at<float>(r, c);
  std::vector<int> m12(pKF1.mvKeys.size(), -1);
  int nm = 0;
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (cms_search_for_triangulation(ctx, &k1, &k2, e, mbCheckOrientation ? 1 : 0, m12.data(), &nm) != CMS_OK)
      throw std::runtime_error(std::string("cms_search_for_triangulation: ") + cms_last_error());
  }
  vMatchedPairs.reserve(nm);
  for (size_t i = 0; i < m12.size(); ++i) if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair(i, (size_t)m12[i]));
  return nm;
}

int ORBMatcher::SearchByBoW(const KeyFrameView& pKF, FrameView& F, std::vector<long>& vpMapPointMatches) {
  const int N = (int)F.mvKeys.size(), NK = (int)pKF.mvKeys.size();
  vpMapPointMatches.assign(N, -1);
  if (N == 0) return 0;
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  // the key frame as cms_keyframe (key points, descriptors, map-point slots, mFeatVec; rays and pose are not read) and the skip flags
  std::vector<cms_keypoint> kk(NK + 1);
  std::vector<uint8_t> kd(32 * (size_t)NK + 32), skip(NK + 1, 0);
  std::vector<int> kmp(NK + 1), nid, noff(1, 0), nfeat;
  for (int i = 0; i < NK; ++i) {
    const cv::KeyPoint& k = pKF.mvKeys[i];
    kk[i].x = k.pt.x; kk[i].y = k.pt.y; kk[i].size = k.size; kk[i].angle = k.angle; kk[i].response = k.response; kk[i].octave = k.octave;
    std::memcpy(&kd[32 * (size_t)i], pKF.mDescriptors.ptr<uint8_t>(i), 32);
    kmp[i] = pKF.mvpMapPoints[i] >= 0 ? 1 : -1;
    skip[i] = i < (int)pKF.mvbMapPointBad.size() ? pKF.mvbMapPointBad[i] : 0;
  }
  for (const auto& e : pKF.mFeatVec) {
    nid.push_back((int)e.first);
    for (unsigned f : e.second) nfeat.push_back((int)f);
    noff.push_back((int)nfeat.size());
  }
  cms_keyframe k{};
  k.n = NK; k.kps = kk.data(); k.desc = kd.data(); k.mp = kmp.data();
  k.nnodes = (int)nid.size(); k.node_id = nid.data(); k.node_off = noff.data(); k.node_feat = nfeat.data();
  // the frame: key points and descriptors into row 0 of the shared context, FeatureVector from the host
  std::vector<cms_keypoint> fk(N);
  std::vector<uint8_t> fd(32 * (size_t)N);
  for (int i = 0; i < N; ++i) {
    const cv::KeyPoint& q = F.mvKeys[i];
    fk[i].x = q.pt.x; fk[i].y = q.pt.y; fk[i].size = q.size; fk[i].angle = q.angle; fk[i].response = q.response; fk[i].octave = q.octave;
    std::memcpy(&fd[32 * (size_t)i], F.mDescriptors.ptr<uint8_t>(i), 32);
  }
  std::vector<int> fid, foff(1, 0), ffeat;
  for (const auto& e : F.mFeatVec) {
    fid.push_back((int)e.first);
    for (unsigned f : e.second) ffeat.push_back((int)f);
    foff.push_back((int)ffeat.size());
  }
  std::vector<int> kf_idx(N, -1);
  int nm = 0;
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    int rc = cms_area_set_keypoints(ctx, 0, N, fk.data());
    if (rc == CMS_OK) rc = cms_area_set_descriptors(ctx, 0, N, fd.data());
    if (rc == CMS_OK) rc = cms_search_by_bow(ctx, 0, N, (int)fid.size(), fid.data(), foff.data(), ffeat.data(), &k, skip.data(), mfNNratio,
                                             mbCheckOrientation ? 1 : 0, kf_idx.data(), &nm);
    if (rc != CMS_OK) throw std::runtime_error(std::string("cms_search_by_bow: ") + cms_last_error());
  }
  for (int i = 0; i < N; ++i) if (kf_idx[i] >= 0) vpMapPointMatches[i] = pKF.mvpMapPoints[kf_idx[i]];
  return nm;
}

int ORBMatcher::SearchByBoW(const KeyFrameView& pKF1, const KeyFrameView& pKF2, std::vector<long>& vpMatches12) {
  const int N1 = (int)pKF1.mvKeys.size(), N2 = (int)pKF2.mvKeys.size();
  vpMatches12.assign(N1, -1);
  if (N1 == 0 || N2 == 0) return 0;
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  // a view as cms_keyframe (key points, descriptors, map-point slots, mFeatVec; the search reads neither rays nor pose) and its skip flags
  struct Side { KfPack p; std::vector<uint8_t> skip; cms_keyframe k; };
  auto pack = [](const KeyFrameView& kf, Side& s) {
    const int N = (int)kf.mvKeys.size();
    KeyFrameView v;
    v.mvKeys = kf.mvKeys; v.mDescriptors = kf.mDescriptors; v.mvpMapPoints = kf.mvpMapPoints; v.mFeatVec = kf.mFeatVec;
    v.mvKeyRays.assign(N, cv::Vec3f());
    float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    v.Tcw = cv::Mat(4, 4, cv::CV_32F, eye, 16);
    s.k = pack_keyframe(v, s.p);
    s.skip.assign(N + 1, 0);
    for (int i = 0; i < N && i < (int)kf.mvbMapPointBad.size(); ++i) s.skip[i] = kf.mvbMapPointBad[i];
  };
  Side s1, s2;
  pack(pKF1, s1); pack(pKF2, s2);
  std::vector<int> idx2(N1, -1);
  int nm = 0;
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!g_bow_kf_store && cms_kfstore_create(&g_bow_kf_store, ctx, 2, 4096, 4096) != CMS_OK)
      throw std::runtime_error(std::string("cms_kfstore_create: ") + cms_last_error());
    cms_bow_kf_job q;
    q.slot1 = 0; q.n1 = N1; q.slot2 = 1; q.n2 = N2; q.skip1 = s1.skip.data(); q.skip2 = s2.skip.data();
    int rc = cms_kfstore_put(g_bow_kf_store, 0, &s1.k);
    if (rc == CMS_OK) rc = cms_kfstore_put(g_bow_kf_store, 1, &s2.k);
    if (rc == CMS_OK) rc = cms_kfstore_search_by_bow_keyframes(g_bow_kf_store, ctx, 1, &q, mfNNratio, mbCheckOrientation ? 1 : 0, idx2.data(), &nm);
    if (rc != CMS_OK) throw std::runtime_error(std::string("cms_kfstore_search_by_bow_keyframes: ") + cms_last_error());
  }
  for (int i = 0; i < N1; ++i) if (idx2[i] >= 0) vpMatches12[i] = pKF2.mvpMapPoints[idx2[i]];
  return nm;
}

int ORBMatcher::SearchBySim3(const KeyFrameView& pKF1, const KeyFrameView& pKF2, std::vector<long>& vpMatches12, float s12, const cv::Mat& R12, const cv::Mat& t12,
                             float th, bool zAsWritten) {
  const int N1 = (int)pKF1.mvKeys.size(), N2 = (int)pKF2.mvKeys.size();
  if ((int)vpMatches12.size() != N1) throw std::runtime_error("SearchBySim3: vpMatches12 must have one entry per key point of pKF1");
  if ((int)pKF1.mvMapPoints.size() != N1 || (int)pKF2.mvMapPoints.size() != N2) throw std::runtime_error("SearchBySim3: mvMapPoints must have one entry per key point");
  if (R12.rows != 3 || R12.cols != 3 || R12.type() != cv::CV_32F || t12.rows != 3 || t12.cols != 1 || t12.type() != cv::CV_32F)
    throw std::runtime_error("SearchBySim3: R12 must be 3x3 and t12 3x1, CV_32F");
  if (N1 == 0 || N2 == 0) return 0;
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  // :1387-1400 on ids: a key point of pKF1 that holds a match already, and the key point of pKF2 that observes the matched point (GetIndexInKeyFrame)
  std::vector<uint8_t> matched1(N1, 0), matched2(N2, 0);
  std::map<long, int> index_in_kf2;
  for (int i = N2 - 1; i >= 0; --i) if (pKF2.mvpMapPoints[i] >= 0) index_in_kf2[pKF2.mvpMapPoints[i]] = i;
  for (int i = 0; i < N1; ++i) {
    if (vpMatches12[i] < 0) continue;
    matched1[i] = 1;
    const auto it = index_in_kf2.find(vpMatches12[i]);
    if (it != index_in_kf2.end()) matched2[it->second] = 1;
  }
  // a view as cms_keyframe (key points, descriptors, pose; the search reads neither rays nor the FeatureVector) and its map-point records
  const int M = N1 + N2;
  std::vector<uint8_t> skip(M, 1), mpd(32 * (size_t)M, 0);
  std::vector<float> pos(3 * (size_t)M, 0.0f), dmin(M, 0.0f), dmax(M, 0.0f);
  struct Side { KfPack p; cms_keyframe k; };
  auto pack = [&](const KeyFrameView& kf, const std::vector<uint8_t>& matched, int at, Side& s) {
    const int N = (int)kf.mvKeys.size();
    KeyFrameView v;
    v.mvKeys = kf.mvKeys; v.mDescriptors = kf.mDescriptors; v.mvpMapPoints = kf.mvpMapPoints; v.Tcw = kf.Tcw;
    v.mvKeyRays.assign(N, cv::Vec3f());
    s.k = pack_keyframe(v, s.p);
    for (int i = 0; i < N; ++i) {
      if (kf.mvpMapPoints[i] < 0 || matched[i] || (i < (int)kf.mvbMapPointBad.size() && kf.mvbMapPointBad[i])) continue;      // !pMP || vbAlreadyMatched[i] || pMP->isBad()
      const MapPointView& mp = kf.mvMapPoints[i];
      const size_t r = (size_t)at + i;
      skip[r] = 0;
      for (int c = 0; c < 3; ++c) pos[3 * r + c] = mp.mWorldPos.at<float>(c, 0);
      dmin[r] = mp.mfMinDistance; dmax[r] = mp.mfMaxDistance;
      std::memcpy(&mpd[32 * r], mp.mDescriptor.ptr<uint8_t>(0), 32);
    }
  };
  Side s1, s2;
  pack(pKF1, matched1, 0, s1); pack(pKF2, matched2, N1, s2);
  cms_sim3_search_job q;
  q.slot1 = 0; q.n1 = N1; q.slot2 = 1; q.n2 = N2; q.s12 = s12; q.off1 = 0; q.off2 = N1;
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) q.R12[3 * r + c] = R12.at<float>(r, c); q.t12[r] = t12.at<float>(r, 0); }
  std::vector<int> idx2(N1, -1);
  int nFound = 0;
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!g_bow_kf_store && cms_kfstore_create(&g_bow_kf_store, ctx, 2, 4096, 4096) != CMS_OK)
      throw std::runtime_error(std::string("cms_kfstore_create: ") + cms_last_error());
    int rc = cms_kfstore_put(g_bow_kf_store, 0, &s1.k);
    if (rc == CMS_OK) rc = cms_kfstore_put(g_bow_kf_store, 1, &s2.k);
    if (rc == CMS_OK) rc = cms_kfstore_search_by_sim3(g_bow_kf_store, ctx, 1, &q, M, skip.data(), pos.data(), dmin.data(), dmax.data(), mpd.data(), th, zAsWritten ? 1 : 0,
                                                      idx2.data(), &nFound);
    if (rc != CMS_OK) throw std::runtime_error(std::string("cms_kfstore_search_by_sim3: ") + cms_last_error());
  }
  for (int i = 0; i < N1; ++i) if (idx2[i] >= 0) vpMatches12[i] = pKF2.mvpMapPoints[idx2[i]];      // :1579
  return nFound;
}

namespace {
// what the two Scw matchers share: the view in slot 0 of the shared context's small store, the points as ONE set, one job
struct Sim3ProjCall {
  std::vector<float> pos, nrm, dmin, dmax;
  std::vector<uint8_t> desc, skip;
  cms_sim3_proj_job q;
  int set_off[2];
  KfPack pack;
  cms_keyframe k;
  Sim3ProjCall(const char* who, const KeyFrameView& kf, const cv::Mat& Scw, const std::vector<MapPointView>& pts) {
    const int N = (int)kf.mvKeys.size(), M = (int)pts.size();
    if (Scw.type() != cv::CV_32F || Scw.cols != 4 || (Scw.rows != 4 && Scw.rows != 3)) throw std::runtime_error(std::string(who) + ": Scw must be 4x4 (or 3x4) CV_32F");
    pos.resize(3 * (size_t)M + 3); nrm.resize(3 * (size_t)M + 3); dmin.resize(M + 1); dmax.resize(M + 1); desc.resize(32 * (size_t)M + 32); skip.assign(M + 1, 0);
    for (int i = 0; i < M; ++i) {
      for (int c = 0; c < 3; ++c) { pos[3 * (size_t)i + c] = pts[i].mWorldPos.at<float>(c, 0); nrm[3 * (size_t)i + c] = pts[i].mNormalVector.at<float>(c, 0); }
      dmin[i] = pts[i].mfMinDistance; dmax[i] = pts[i].mfMaxDistance;
      std::memcpy(&desc[32 * (size_t)i], pts[i].mDescriptor.ptr<uint8_t>(0), 32);
    }
    KeyFrameView v;
    v.mvKeys = kf.mvKeys; v.mDescriptors = kf.mDescriptors; v.mvpMapPoints = kf.mvpMapPoints;
    v.mvKeyRays.assign(N, cv::Vec3f());
    float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};      // (the search does not read the slot's pose)
    v.Tcw = cv::Mat(4, 4, cv::CV_32F, eye, 16);
    k = pack_keyframe(v, pack);
    q.slot = 0; q.n = N; q.set = 0;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) q.Scw[4 * r + c] = Scw.at<float>(r, c);
    set_off[0] = 0; set_off[1] = M;
  }
};
}  // namespace

int ORBMatcher::SearchByProjection(const KeyFrameView& pKF, const cv::Mat& Scw, const std::vector<MapPointView>& vpPoints, std::vector<long>& vpMatched, int th) {
  const int N = (int)pKF.mvKeys.size(), M = (int)vpPoints.size();
  if ((int)vpMatched.size() != N) throw std::runtime_error("SearchByProjection: vpMatched must have one entry per key point of pKF");
  Sim3ProjCall call("SearchByProjection", pKF, Scw, vpPoints);
  if (N == 0 || M == 0) return 0;
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  std::set<long> spAlreadyFound(vpMatched.begin(), vpMatched.end());      // :806-807
  spAlreadyFound.erase(-1);
  std::vector<uint8_t> taken(N + 1, 0);
  for (int i = 0; i < N; ++i) taken[i] = vpMatched[i] >= 0;
  for (int i = 0; i < M; ++i) call.skip[i] = vpPoints[i].mbBad || spAlreadyFound.count(vpPoints[i].mnId);      // :817
  std::vector<int> match(M, -1);
  int nmatches = 0;
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!g_bow_kf_store && cms_kfstore_create(&g_bow_kf_store, ctx, 2, 4096, 4096) != CMS_OK)
      throw std::runtime_error(std::string("cms_kfstore_create: ") + cms_last_error());
    int rc = cms_kfstore_put(g_bow_kf_store, 0, &call.k);
    if (rc == CMS_OK) rc = cms_kfstore_search_by_projection_sim3(g_bow_kf_store, ctx, 1, call.set_off, call.pos.data(), call.nrm.data(), call.dmin.data(), call.dmax.data(),
                                                                 call.desc.data(), 1, &call.q, call.skip.data(), taken.data(), (float)th, match.data(), &nmatches);
    if (rc != CMS_OK) throw std::runtime_error(std::string("cms_kfstore_search_by_projection_sim3: ") + cms_last_error());
  }
  for (int i = 0; i < M; ++i) if (match[i] >= 0) vpMatched[match[i]] = vpPoints[i].mnId;      // :896
  return nmatches;
}

int ORBMatcher::Fuse(KeyFrameView& pKF, const cv::Mat& Scw, const std::vector<MapPointView>& vpPoints, float th, std::vector<long>& vpReplacePoint) {
  const int N = (int)pKF.mvKeys.size(), M = (int)vpPoints.size();
  if ((int)vpReplacePoint.size() != M) throw std::runtime_error("Fuse: vpReplacePoint must have one entry per point");
  Sim3ProjCall call("Fuse", pKF, Scw, vpPoints);
  if (N == 0 || M == 0) return 0;
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  auto bad_at = [&](int i) { return i < (int)pKF.mvbMapPointBad.size() && pKF.mvbMapPointBad[i]; };
  std::set<long> spAlreadyFound;                                            // pKF->GetMapPoints(): the key frame's points that are not bad (:1256)
  for (int i = 0; i < N; ++i) if (pKF.mvpMapPoints[i] >= 0 && !bad_at(i)) spAlreadyFound.insert(pKF.mvpMapPoints[i]);
  for (int i = 0; i < M; ++i) call.skip[i] = vpPoints[i].mbBad || spAlreadyFound.count(vpPoints[i].mnId);      // :1268
  std::vector<int> bi(M, -1), bd(M, 256);
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!g_bow_kf_store && cms_kfstore_create(&g_bow_kf_store, ctx, 2, 4096, 4096) != CMS_OK)
      throw std::runtime_error(std::string("cms_kfstore_create: ") + cms_last_error());
    int rc = cms_kfstore_put(g_bow_kf_store, 0, &call.k);
    if (rc == CMS_OK) rc = cms_kfstore_fuse_search_sim3(g_bow_kf_store, ctx, 1, call.set_off, call.pos.data(), call.nrm.data(), call.dmin.data(), call.dmax.data(),
                                                        call.desc.data(), 1, &call.q, call.skip.data(), th, bi.data(), bd.data());
    if (rc != CMS_OK) throw std::runtime_error(std::string("cms_kfstore_fuse_search_sim3: ") + cms_last_error());
  }
  int nFused = 0;
  for (int i = 0; i < M; ++i) {                                             // :1345-1359 in list order
    if (bi[i] < 0) continue;
    const long pMPinKF = pKF.mvpMapPoints[bi[i]];
    if (pMPinKF >= 0) {
      if (!bad_at(bi[i])) vpReplacePoint[i] = pMPinKF;
    } else {
      pKF.mvpMapPoints[bi[i]] = vpPoints[i].mnId;                           // pMP->AddObservation(pKF,bestIdx); pKF->AddMapPoint(pMP,bestIdx);
      if (bi[i] < (int)pKF.mvbMapPointBad.size()) pKF.mvbMapPointBad[bi[i]] = 0;
    }
    ++nFused;
  }
  return nFused;
}

int ORBMatcher::SearchByProjection(FrameView& CurrentFrame, const KeyFrameView& pKF, const std::set<long>& sAlreadyFound, float th, int ORBdist) {
  const int N = (int)CurrentFrame.mvKeys.size(), NK = (int)pKF.mvKeys.size();
  if (N == 0) return 0;
  if (CurrentFrame.mTcw.rows != 4 || CurrentFrame.mTcw.cols != 4 || CurrentFrame.mTcw.type() != cv::CV_32F) throw std::runtime_error("SearchByProjection: mTcw must be 4x4 CV_32F");
  if ((int)pKF.mvMapPoints.size() != NK) throw std::runtime_error("SearchByProjection: pKF.mvMapPoints must have one entry per key point");
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  float pose12[12];
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) pose12[3 * r + c] = CurrentFrame.mTcw.at<float>(r, c); pose12[9 + r] = CurrentFrame.mTcw.at<float>(r, 3); }
  // the list of :268-276: a map point, not bad, not already found -- in key-point order
  std::vector<int> feat;
  for (int i = 0; i < NK; ++i) {
    const long id = pKF.mvpMapPoints[i];
    if (id < 0 || (i < (int)pKF.mvbMapPointBad.size() && pKF.mvbMapPointBad[i]) || sAlreadyFound.count(id)) continue;
    feat.push_back(i);
  }
  const int M = (int)feat.size();
  if (M == 0) return 0;
  std::vector<float> ang(M), pos(3 * (size_t)M), dmin(M), dmax(M);
  std::vector<uint8_t> mpd(32 * (size_t)M);
  for (int k = 0; k < M; ++k) {
    const MapPointView& mp = pKF.mvMapPoints[feat[k]];
    ang[k] = pKF.mvKeys[feat[k]].angle;
    for (int c = 0; c < 3; ++c) pos[3 * (size_t)k + c] = mp.mWorldPos.at<float>(c, 0);
    dmin[k] = mp.mfMinDistance; dmax[k] = mp.mfMaxDistance;
    std::memcpy(&mpd[32 * (size_t)k], mp.mDescriptor.ptr<uint8_t>(0), 32);
  }
  std::vector<cms_keypoint> kps(N);
  std::vector<uint8_t> tdesc(32 * (size_t)N);
  std::vector<int> kp_mp(N, -1), match(M, -1);
  for (int j = 0; j < N; ++j) {
    const cv::KeyPoint& k = CurrentFrame.mvKeys[j];
    kps[j].x = k.pt.x; kps[j].y = k.pt.y; kps[j].size = k.size; kps[j].angle = k.angle; kps[j].response = k.response; kps[j].octave = k.octave;
    std::memcpy(&tdesc[32 * (size_t)j], CurrentFrame.mDescriptors.ptr<uint8_t>(j), 32);
    if (CurrentFrame.mvpMapPoints[j] >= 0) kp_mp[j] = 0x40000000;      // any map point (:320), no Observations() test
  }
  int nm = 0;
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    int rc = cms_area_set_keypoints(ctx, 0, N, kps.data());
    if (rc == CMS_OK) rc = cms_area_set_descriptors(ctx, 0, N, tdesc.data());
    if (rc == CMS_OK) rc = cms_area_grid(ctx, 1);
    if (rc == CMS_OK) rc = cms_search_by_projection_keyframe(ctx, 0, pose12, M, ang.data(), pos.data(), dmin.data(), dmax.data(), mpd.data(), th, ORBdist,
                                                            mbCheckOrientation ? 1 : 0, N, kp_mp.data(), match.data(), &nm);
    if (rc != CMS_OK) throw std::runtime_error(std::string("cms_search_by_projection_keyframe: ") + cms_last_error());
  }
  for (int k = 0; k < M; ++k) if (match[k] >= 0) CurrentFrame.mvpMapPoints[match[k]] = pKF.mvpMapPoints[feat[k]];
  return nm;
}

int ORBMatcher::SearchByProjection(FrameView& Cur, const FrameView& Last, float th, bool) {
  const int N2 = (int)Cur.mvKeys.size();
  if (!Last.mvMapPointPos.empty() && Cur.mTcw.rows == 4 && Cur.mTcw.cols == 4 && N2 > 0) {
    // the whole function on the device (cms_search_by_projection)
    const int NL = (int)Last.mvKeys.size();
    cms_ctx* dctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
    float pose12[12];
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) pose12[3 * r + c] = Cur.mTcw.at<float>(r, c); pose12[9 + r] = Cur.mTcw.at<float>(r, 3); }
    std::vector<uint8_t> valid(NL), mpd(32 * (size_t)NL), tdesc(32 * (size_t)N2);
    std::vector<float> Xw(3 * (size_t)NL), ang(NL);
    std::vector<int> oct(NL), kp_mp(N2, -1), match(NL, -1);
    for (int i = 0; i < NL; ++i) {
      valid[i] = Last.mvpMapPoints[i] >= 0 && !(i < (int)Last.mvbOutlier.size() && Last.mvbOutlier[i]);
      for (int c = 0; c < 3; ++c) Xw[3 * (size_t)i + c] = Last.mvMapPointPos[i].v[c];
      oct[i] = Last.mvKeys[i].octave; ang[i] = Last.mvKeys[i].angle;
      std::memcpy(&mpd[32 * (size_t)i], Last.mMapPointDescriptors.ptr<uint8_t>(i), 32);
    }
    std::vector<cms_keypoint> kps(N2);
    for (int j = 0; j < N2; ++j) {
      const cv::KeyPoint& k = Cur.mvKeys[j];
      kps[j].x = k.pt.x; kps[j].y = k.pt.y; kps[j].size = k.size; kps[j].angle = k.angle; kps[j].response = k.response; kps[j].octave = k.octave;
      std::memcpy(&tdesc[32 * (size_t)j], Cur.mDescriptors.ptr<uint8_t>(j), 32);
      if (Cur.mvpMapPoints[j] >= 0) kp_mp[j] = 0x40000000;
    }
    int nm = 0;
    {
      std::lock_guard<std::mutex> lock(g_ctx_mutex);
      int rc = cms_area_set_keypoints(dctx, 0, N2, kps.data());
      if (rc == CMS_OK) rc = cms_area_set_descriptors(dctx, 0, N2, tdesc.data());
      if (rc == CMS_OK) rc = cms_area_grid(dctx, 1);
      if (rc == CMS_OK) rc = cms_search_by_projection(dctx, 0, pose12, NL, valid.data(), Xw.data(), oct.data(), ang.data(), mpd.data(), th, mbCheckOrientation ? 1 : 0,
                                                     TH_HIGH, N2, kp_mp.data(), match.data(), &nm);
      if (rc != CMS_OK) throw std::runtime_error(std::string("cms_search_by_projection: ") + cms_last_error());
    }
    for (int i = 0; i < NL; ++i) if (match[i] >= 0) Cur.mvpMapPoints[match[i]] = Last.mvpMapPoints[i];
    return nm;
  }
  cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast);
  // candidate windows: CurrentFrame.GetFeaturesInArea(u, v, th * scale[octave], octave - 1, octave + 1) (ORBMatcher.cpp:176-181) for
  // every projected map point of the last frame, answered on the device by the frame grid of the current frame's key points --
  // same unfolding cases, same candidate order as Frame.cpp:251-716
  std::vector<int> qall;
  std::vector<float> qx, qy, qr;
  std::vector<int> qlo, qhi;
  for (int i = 0; i < (int)Last.mvKeys.size(); ++i) {
    if (Last.mvpMapPoints[i] < 0 || (i < (int)Last.mvbOutlier.size() && Last.mvbOutlier[i])) continue;
    const cv::Point2f p = Last.projInCurrent[i];
    if (p.x < 0 || p.y < 0) continue;
    const int oct = Last.mvKeys[i].octave;
    qall.push_back(i); qx.push_back(p.x); qy.push_back(p.y); qr.push_back(th * Cur.mvScaleFactors[oct]);
    qlo.push_back(oct - 1); qhi.push_back(oct + 1);
  }
  std::vector<int> qidx, off(1, 0), cand;
  if (!qall.empty()) {
    std::vector<cms_keypoint> kps(N2);
    for (int j = 0; j < N2; ++j) {
      const cv::KeyPoint& k = Cur.mvKeys[j];
      kps[j].x = k.pt.x; kps[j].y = k.pt.y; kps[j].size = k.size; kps[j].angle = k.angle; kps[j].response = k.response; kps[j].octave = k.octave;
    }
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    std::vector<int> aoff(qall.size() + 1), aidx(64 * qall.size() + 1024);
    int total = 0;
    int rc = cms_area_set_keypoints(ctx, 0, N2, kps.data());
    if (rc == CMS_OK) rc = cms_area_grid(ctx, 1);
    if (rc == CMS_OK) rc = cms_features_in_area(ctx, 0, (int)qall.size(), qx.data(), qy.data(), qr.data(), qlo.data(), qhi.data(), aoff.data(),
                                                aidx.data(), (int)aidx.size(), &total);
    if (rc == CMS_ERR_OVERFLOW) {               // denser than 64 candidates per window: retry with the exact size
      aidx.resize((size_t)total + 1);
      rc = cms_features_in_area(ctx, 0, (int)qall.size(), qx.data(), qy.data(), qr.data(), qlo.data(), qhi.data(), aoff.data(), aidx.data(),
                                (int)aidx.size(), &total);
    }
    if (rc != CMS_OK) throw std::runtime_error(std::string("cms_features_in_area: ") + cms_last_error());
    for (size_t q = 0; q < qall.size(); ++q) {
      if (aoff[q + 1] == aoff[q]) continue;     // vIndices2.empty()
      qidx.push_back(qall[q]);
      cand.insert(cand.end(), aidx.begin() + aoff[q], aidx.begin() + aoff[q + 1]);
      off.push_back((int)cand.size());
    }
  }
  const int nq = (int)qidx.size();
  if (nq == 0) return 0;
  std::vector<uint8_t> qdesc((size_t)nq * 32), excl(N2, 0);
  for (int q = 0; q < nq; ++q) std::memcpy(&qdesc[(size_t)q * 32], Last.mDescriptors.ptr<uint8_t>(qidx[q]), 32);
  for (int j = 0; j < N2; ++j) excl[j] = Cur.mvpMapPoints[j] >= 0;
  std::vector<uint8_t> tdesc((size_t)N2 * 32);
  for (int j = 0; j < N2; ++j) std::memcpy(&tdesc[(size_t)j * 32], Cur.mDescriptors.ptr<uint8_t>(j), 32);
  std::vector<int> bi(nq), bd(nq), sd(nq);
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (cms_hamming_best2(ctx, qdesc.data(), nq, tdesc.data(), N2, off.data(), cand.data(), nullptr, excl.data(), bi.data(), bd.data(),
                          nullptr, sd.data(), nullptr) != CMS_OK)
      throw std::runtime_error(std::string("cms_hamming_best2: ") + cms_last_error());
  }
  // greedy replay in the reference's order (ORBMatcher.cpp:150-222)
  const int nBins = (int)std::ceil(360.0f / HISTO_LENGTH);
  std::vector<std::vector<int>> rotHist(nBins);
  const float factor = 1.0f / HISTO_LENGTH;
  int nmatches = 0;
  for (int q = 0; q < nq; ++q) {
    int bestIdx = bi[q], bestDist = bd[q];
    if (bestIdx >= 0 && Cur.mvpMapPoints[bestIdx] >= 0 && !excl[bestIdx]) {   // taken earlier in THIS call: rescan on the host
      bestDist = 256; bestIdx = -1;
      for (int c = off[q]; c < off[q + 1]; ++c) {
        const int j = cand[c];
        if (Cur.mvpMapPoints[j] >= 0) continue;
        const int d = DescriptorDistance(Last.mDescriptors.row(qidx[q]), Cur.mDescriptors.row(j));
        if (d < bestDist) { bestDist = d; bestIdx = j; }
      }
    }
    if (bestIdx < 0 || bestDist > TH_HIGH) continue;
    Cur.mvpMapPoints[bestIdx] = Last.mvpMapPoints[qidx[q]];
    ++nmatches;
    if (mbCheckOrientation) {
      float rot = Last.mvKeys[qidx[q]].angle - Cur.mvKeys[bestIdx].angle;
      if (rot < 0.0) rot += 360.0f;
      int bin = (int)std::round(rot * factor);
      if (bin == nBins) bin = 0;
      rotHist[bin].push_back(bestIdx);
    }
  }
  if (mbCheckOrientation) {   // ComputeThreeMaxima (ORBMatcher.cpp:905-946)
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < nBins; ++i) {
      const int s = (int)rotHist[i].size();
      if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
      else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
      else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) ind3 = -1;
    for (int i = 0; i < nBins; ++i)
      if (i != ind1 && i != ind2 && i != ind3)
        for (int j : rotHist[i]) { Cur.mvpMapPoints[j] = -1; --nmatches; }
  }
  return nmatches;
}

// ------------------------------------------------------------------------------------------------ local BA
static void R_to_quat(const double m[9], double* q) {  // Eigen::Quaterniond(Matrix3d), as Converter::toSE3Quat uses it
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = std::sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + 1.0); q[i] = 0.5 * t; t = 0.5 / t;
    q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t; q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t; q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
  }
}
void System::SaveKeyFrameTrajectoryTUM(const std::string& filename, const std::vector<TrajectoryKeyFrame>& vpKFs) {
  std::ofstream f(filename.c_str());
  f << std::fixed;
  for (const TrajectoryKeyFrame& kf : vpKFs) {
    if (kf.bad) continue;
    double Rt[9];                                           // R^T = GetRotation().t(), through Converter::toMatrix3d (float -> double)
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rt[3 * r + c] = kf.Tcw.at<float>(c, r);
    double q[4];
    R_to_quat(Rt, q);                                       // Eigen::Quaterniond(Matrix3d), stored as float (Converter.cpp:141-153)
    float t[3];                                             // KeyFrame::GetCameraCenter() = -R^T t in float arithmetic (KeyFrame.cpp SetPose)
    for (int r = 0; r < 3; ++r) {
      float acc = 0.f;
      for (int c = 0; c < 3; ++c) acc += kf.Tcw.at<float>(c, r) * kf.Tcw.at<float>(c, 3);
      t[r] = -acc;
    }
    f << std::setprecision(6) << kf.mTimeStamp << std::setprecision(7) << " " << t[0] << " " << t[1] << " " << t[2] << " " << (float)q[0] << " "
      << (float)q[1] << " " << (float)q[2] << " " << (float)q[3] << std::endl;
  }
}

int Optimizer::PoseOptimization(PoseFrame* fr) {
  CamModelGeneral* cam = CamModelGeneral::GetCamera();
  const int N = fr->N;
  fr->mvbOutlier.resize(N);
  std::vector<double> Xw, obs, inv;
  std::vector<int8_t> face;
  std::vector<int> index;
  int nInitialCorrespondences = 0;
  for (int i = 0; i < N; ++i) {
    if (fr->mvKeyRays[i](2) < cam->GetCosFovTh()) continue;                      // Optimizer.cpp:83-85
    if (!fr->mvbHasMapPoint[i]) continue;
    ++nInitialCorrespondences;
    fr->mvbOutlier[i] = false;
    const cv::KeyPoint& kp = fr->mvKeys[i];
    const int f = cam->FaceInCubemap(kp.pt);                                      // :103
    if (f == CamModelGeneral::UNKNOWN_FACE) throw std::runtime_error("PoseOptimization: key point on an unknown face");   // the reference exits
    double u, v;
    cam->GetPosInFace(u, v, (double)kp.pt.x, (double)kp.pt.y);                     // :104-106
    obs.push_back(u); obs.push_back(v);
    inv.push_back((double)fr->mvInvLevelSigma2[kp.octave]);                        // :107-108
    face.push_back((int8_t)f);
    for (int k = 0; k < 3; ++k) Xw.push_back((double)fr->mvMapPointPos[i](k));     // :118-121
    index.push_back(i);
  }
  if (nInitialCorrespondences < 3) return 0;                                       // :131-132
  double pose[7], R[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[3 * r + c] = fr->mTcw.at<float>(r, c);   // Converter::toSE3Quat
  for (int r = 0; r < 3; ++r) pose[r] = fr->mTcw.at<float>(r, 3);
  R_to_quat(R, pose + 3);
  const int n = (int)index.size();
  std::vector<uint8_t> out(n);
  int ninl = 0;
  const double f = cam->Get_fx();
  const int rc = cms_pose_optimize(0, n, Xw.data(), obs.data(), inv.data(), face.data(), f, f, f, f, pose, out.data(), &ninl, nullptr);
  if (rc < 0) throw std::runtime_error(std::string("cms_pose_optimize: ") + cms_last_error());
  for (int e = 0; e < n; ++e) fr->mvbOutlier[index[e]] = out[e] != 0;
  const double x = pose[3], y = pose[4], z = pose[5], w = pose[6];                  // Converter::toCvMat(SE3Quat) -> float 4x4
  const double Ro[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                        2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) fr->mTcw.at<float>(r, c) = (float)Ro[3 * r + c]; fr->mTcw.at<float>(r, 3) = (float)pose[r]; }
  return ninl;
}

void Optimizer::LocalBundleAdjustment(LocalBAWindow* win, bool* pbStopFlag) {
  CamModelGeneral* cam = CamModelGeneral::GetCamera();
  const int K = (int)win->keyframes.size(), P = (int)win->mappoints.size();
  win->toErase.clear();
  if (K == 0 || P == 0) return;
  std::vector<double> poses((size_t)K * 7), points((size_t)P * 3);
  std::vector<uint8_t> fixed(K);
  for (int k = 0; k < K; ++k) {   // Converter::toSE3Quat (Converter.cpp:41-51): float Tcw -> double R, t -> quaternion
    const cv::Mat& T = win->keyframes[k].Tcw;
    double R[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[3 * r + c] = T.at<float>(r, c);
    for (int r = 0; r < 3; ++r) poses[7 * k + r] = T.at<float>(r, 3);
    R_to_quat(R, &poses[7 * k + 3]);
    fixed[k] = (win->keyframes[k].mnId == 0) || win->keyframes[k].fixed;   // Optimizer.cpp:268, 281
  }
  std::vector<int> e_pose, e_point;
  std::vector<double> e_obs, e_inv;
  std::vector<int8_t> e_face;
  std::vector<std::pair<int, int>> e_src;
  for (int p = 0; p < P; ++p) {
    const LocalBAWindow::MP& mp = win->mappoints[p];
    for (int i = 0; i < 3; ++i) points[3 * p + i] = mp.Xw.at<float>(i, 0);   // Converter::toVector3d
    for (const LocalBAWindow::Obs& ob : mp.observations) {
      if (ob.ray(2) < cam->GetCosFovTh()) continue;                            // Optimizer.cpp:323-325
      const int face = cam->FaceInCubemap(ob.kp.pt);                           // :335
      if (face == CamModelGeneral::UNKNOWN_FACE) continue;                     // would exit() inside g2o (edge h:103-108)
      double u, v;
      cam->GetPosInFace(u, v, (double)ob.kp.pt.x, (double)ob.kp.pt.y);          // :336-338
      e_pose.push_back(ob.kf); e_point.push_back(p); e_obs.push_back(u); e_obs.push_back(v);
      e_inv.push_back((double)win->keyframes[ob.kf].mvInvLevelSigma2[ob.kp.octave]);   // :339-340
      e_face.push_back((int8_t)face);
      e_src.push_back(std::make_pair(ob.kf, p));
    }
  }
  const int E = (int)e_pose.size();
  if (E == 0) return;
  if (pbStopFlag && *pbStopFlag) return;                                       // :359-361
  std::vector<uint8_t> flags(E);
  const double f = cam->Get_fx();
  const int rc = cms_ba_run(0, K, poses.data(), fixed.data(), P, points.data(), E, e_pose.data(), e_point.data(), e_obs.data(), e_inv.data(),
                            e_face.data(), f, f, f, f, 5, 10, reinterpret_cast<const volatile uint8_t*>(pbStopFlag), flags.data(), nullptr);
  if (rc < 0) throw std::runtime_error(std::string("cms_ba_run: ") + cms_last_error());
  if (rc == 1) return;
  for (int e = 0; e < E; ++e) if (flags[e]) win->toErase.push_back(e_src[e]);  // :399-412
  for (int k = 0; k < K; ++k) {   // Converter::toCvMat(SE3Quat) -> float 4x4 (Converter.cpp:53-104)
    if (fixed[k]) continue;       // the reference rewrites local key frames only (:432-438); fixed ones are unchanged anyway
    const double* q = &poses[7 * k + 3];
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                         2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    cv::Mat& T = win->keyframes[k].Tcw;
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T.at<float>(r, c) = (float)R[3 * r + c]; T.at<float>(r, 3) = (float)poses[7 * k + r]; }
  }
  for (int p = 0; p < P; ++p)
    for (int i = 0; i < 3; ++i) win->mappoints[p].Xw.at<float>(i, 0) = (float)points[3 * p + i];
}


// ------------------------------------------------------------------------------------------------ Optimizer::GlobalBundleAdjustemnt (src/Optimizer.cpp:453-621)
GlobalBAGraph Optimizer::CollectGlobalBA(const GlobalBAMap& pMap) {
  CamModelGeneral* cam = CamModelGeneral::GetCamera();
  GlobalBAGraph g;
  const int nAll = (int)pMap.mvpKeyFrames.size(), nKF = pMap.nListedKeyFrames < 0 ? nAll : std::min(pMap.nListedKeyFrames, nAll), nMP = (int)pMap.mvpMapPoints.size();
  g.vbNotIncludedMP.assign((size_t)nMP, 0);
  std::vector<int> slot((size_t)nAll, -1);
  long unsigned int maxKFid = 0;
  for (int i = 0; i < nKF; ++i) {                                                  // :483-495
    const GlobalBAKeyFrameView& kf = pMap.mvpKeyFrames[(size_t)i];
    if (kf.mbBad) continue;
    double R[9], pose[7];                                                          // Converter::toSE3Quat (Converter.cpp:41-51)
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[3 * r + c] = kf.Tcw.at<float>(r, c);
    for (int r = 0; r < 3; ++r) pose[r] = kf.Tcw.at<float>(r, 3);
    R_to_quat(R, pose + 3);
    slot[(size_t)i] = (int)g.vertexKF.size();
    g.vertexKF.push_back(i);
    g.poses.insert(g.poses.end(), pose, pose + 7);
    g.fixed.push_back(kf.mnId == 0 ? 1 : 0);                                       // :491
    if (kf.mnId > maxKFid) maxKFid = kf.mnId;
  }
  for (int i = 0; i < nMP; ++i) {                                                  // :500-568
    const GlobalBAMapPointView& mp = pMap.mvpMapPoints[(size_t)i];
    if (mp.mbBad) continue;
    const int p = (int)g.vertexMP.size();
    const size_t e0 = g.e_pose.size();
    for (const std::pair<int, int>& ob : mp.observations) {
      const GlobalBAKeyFrameView& kf = pMap.mvpKeyFrames[(size_t)ob.first];
      if (kf.mbBad || kf.mnId > maxKFid) continue;                                 // :520
      if (slot[(size_t)ob.first] < 0) continue;                                    // no vertex of that id (the reference would pass g2o a null vertex)
      const cv::KeyPoint& kp = kf.mvKeys[(size_t)ob.second];
      if (kf.mvKeyRays[(size_t)ob.second](2) < cam->GetCosFovTh()) continue;       // :525
      const int face = cam->FaceInCubemap(kp.pt);                                  // :537
      if (face == CamModelGeneral::UNKNOWN_FACE) throw std::runtime_error("GlobalBundleAdjustemnt: key point on an unknown face");      // the reference exits
      double u, v;
      cam->GetPosInFace(u, v, (double)kp.pt.x, (double)kp.pt.y);                    // :538-540
      g.e_pose.push_back(slot[(size_t)ob.first]); g.e_point.push_back(p);
      g.e_obs.push_back(u); g.e_obs.push_back(v);
      g.e_invsig2.push_back((double)kf.mvInvLevelSigma2[(size_t)kp.octave]);       // :541
      g.e_face.push_back((int8_t)face);
    }
    if (g.e_pose.size() == e0) { g.vbNotIncludedMP[(size_t)i] = 1; continue; }     // :559-563
    g.vertexMP.push_back(i);
    for (int c = 0; c < 3; ++c) g.points.push_back((double)mp.Xw.at<float>(c, 0)); // Converter::toVector3d
  }
  return g;
}

void Optimizer::GlobalBundleAdjustemnt(GlobalBAMap& pMap, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust) {
  CamModelGeneral* cam = CamModelGeneral::GetCamera();
  GlobalBAGraph g = CollectGlobalBA(pMap);
  const int K = (int)g.vertexKF.size(), P = (int)g.vertexMP.size(), E = (int)g.e_pose.size();
  if (K > 0 && E > 0) {                                                            // (nothing to optimise: g2o's optimize() returns at once, the estimates are written back as they are)
    const double f = cam->Get_fx();
    cms_ba* ba = nullptr;
    int rc = cms_ba_create(&ba, 0, K, g.poses.data(), g.fixed.data(), P, g.points.data(), E, g.e_pose.data(), g.e_point.data(), g.e_obs.data(), g.e_invsig2.data(),
                           g.e_face.data(), f, f, f, f);
    if (rc < 0) throw std::runtime_error(std::string("cms_ba_create: ") + cms_last_error());
    rc = cms_ba_optimize_global(ba, nIterations, bRobust ? 1 : 0, reinterpret_cast<const volatile uint8_t*>(pbStopFlag), nullptr);      // :570-572
    if (rc >= 0) { const int rr = cms_ba_read(ba, g.poses.data(), g.points.data(), nullptr); if (rr < 0) rc = rr; }
    cms_ba_destroy(ba);
    if (rc < 0) throw std::runtime_error(std::string("cms_ba_optimize_global: ") + cms_last_error());
  }
  for (int k = 0; k < K; ++k) {                                                    // :577-594, Converter::toCvMat(SE3Quat) -> float 4x4 (Converter.cpp:53-104)
    GlobalBAKeyFrameView& kf = pMap.mvpKeyFrames[(size_t)g.vertexKF[(size_t)k]];
    const double* q = &g.poses[7 * (size_t)k + 3];
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                         2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    if (nLoopKF != 0) { if (kf.mTcwGBA.empty()) kf.mTcwGBA = cv::Mat::zeros(4, 4, cv::CV_32F); kf.mnBAGlobalForKF = nLoopKF; }
    cv::Mat& T = nLoopKF == 0 ? kf.Tcw : kf.mTcwGBA;
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T.at<float>(r, c) = (float)R[3 * r + c]; T.at<float>(r, 3) = (float)g.poses[7 * (size_t)k + r]; }
    for (int c = 0; c < 4; ++c) T.at<float>(3, c) = c == 3 ? 1.0f : 0.0f;
  }
  for (int p = 0; p < P; ++p) {                                                    // :597-619
    GlobalBAMapPointView& mp = pMap.mvpMapPoints[(size_t)g.vertexMP[(size_t)p]];
    if (nLoopKF != 0) { if (mp.mPosGBA.empty()) mp.mPosGBA = cv::Mat::zeros(3, 1, cv::CV_32F); mp.mnBAGlobalForKF = nLoopKF; }
    cv::Mat& X = nLoopKF == 0 ? mp.Xw : mp.mPosGBA;
    for (int c = 0; c < 3; ++c) X.at<float>(c, 0) = (float)g.points[3 * (size_t)p + c];
  }
}

// ------------------------------------------------------------------------------------------------ PnPsolver (src/PnPsolver.cpp)
extern "C" int hm_pnp_iterate_host(int F, int njobs, cms_pnp_job* jobs);      // pnp_host.cpp: the host build of csrc/cms_pnp_core.h

PnPsolver::PnPsolver(const FrameView& F, const std::vector<long>& vpMapPointMatches) {
  nMatches_ = vpMapPointMatches.size();
  for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {      // :83-108
    if (vpMapPointMatches[i] < 0) continue;                                  // pMP == NULL
    if (!F.mvbMapPointBad.empty() && F.mvbMapPointBad[i]) continue;          // pMP->isBad()
    const cv::KeyPoint& kp = F.mvKeys[i];
    mvP2D.push_back(kp.pt);
    mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
    mvBearings.push_back(F.mvKeyRays[i]);
    mvP3Dw.push_back(F.mvMapPointPos[i]);
    mvKeyPointIndices.push_back(i);
  }
  draw = [](int min, int max) { const int d = max - min + 1; return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min; };
  SetRansacParameters();
}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2) {
  N = (int)mvBearings.size();
  mRansacMinSet = minSet; mRansacTh2 = th2;
  if (cms_pnp_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, &mRansacMinInliers, &mRansacMaxIts, &mRansacEpsilon))
    throw std::runtime_error(std::string("cms_pnp_ransac_parameters: ") + cms_last_error());
  mvbBestInliers.assign((size_t)N, 0);
}

cv::Mat PnPsolver::find(std::vector<bool>& vbInliers, int& nInliers) {
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
}

cv::Mat PnPsolver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  bNoMore = false; vbInliers.clear(); nInliers = 0;
  if (N < mRansacMinInliers) { bNoMore = true; return cv::Mat(); }      // :175-179
  const int H = std::max(std::max(mRansacMaxIts - mnIterations, nIterations), 0);
  std::vector<int> draws((size_t)H * 4);
  for (int i = 0; i < H; ++i)
    for (int k = 0; k < 4; ++k) draws[(size_t)i * 4 + k] = draw(0, N - k - 1);      // RandomInt(0, vAvailableIndices.size()-1), :195
  std::vector<uint8_t> inliers((size_t)N + 1, 0);
  mvbBestInliers.resize((size_t)N + 1, 0);
  cms_pnp_job q = {};
  q.N = N; q.p3d = N ? &mvP3Dw[0](0) : nullptr; q.p2d = N ? &mvP2D[0].x : nullptr; q.bearing = N ? &mvBearings[0](0) : nullptr; q.sigma2 = mvSigma2.data();
  q.th2 = mRansacTh2; q.min_inliers = mRansacMinInliers; q.max_its = mRansacMaxIts; q.min_set = mRansacMinSet; q.n_iterations = nIterations;
  q.n_draws = (int)draws.size(); q.draws = draws.data();
  q.iterations = mnIterations; q.best_inliers = mnBestInliers; std::memcpy(q.best_Tcw, mBestTcw, sizeof(mBestTcw)); q.best_mask = mvbBestInliers.data();
  q.inliers = inliers.data();
  if (engine == HOST_CORE) {
    const int rc = hm_pnp_iterate_host(CamModelGeneral::GetCamera()->GetCubeFaceWidth(), 1, &q);
    if (rc) throw std::runtime_error("PnPsolver::iterate: the job was refused (" + std::to_string(rc) + ")");
  } else {
    cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures > 0 ? g_ctx_orb.nfeatures : 1000, g_ctx_orb.nfeatures > 0 ? g_ctx_orb.scale_factor : 1.2f,
                                 g_ctx_orb.nfeatures > 0 ? g_ctx_orb.nlevels : 8, g_ctx_orb.nfeatures > 0 ? g_ctx_orb.ini_th_fast : 20,
                                 g_ctx_orb.nfeatures > 0 ? g_ctx_orb.min_th_fast : 7);
    cms_pnp* h = nullptr;
    if (cms_pnp_create(&h, 0, 1, std::max(N, 1), std::max(H, 1))) throw std::runtime_error(std::string("cms_pnp_create: ") + cms_last_error());
    const int rc = cms_pnp_iterate(h, ctx, 1, &q);
    cms_pnp_destroy(h);
    if (rc) throw std::runtime_error(std::string("cms_pnp_iterate: ") + cms_last_error());
  }
  mnIterations = q.iterations; mnBestInliers = q.best_inliers; std::memcpy(mBestTcw, q.best_Tcw, sizeof(mBestTcw));
  bNoMore = q.no_more != 0;
  if (q.status == 0) return cv::Mat();
  nInliers = q.n_inliers;
  vbInliers = std::vector<bool>(nMatches_, false);      // :232-237, :250-255
  for (int i = 0; i < N; i++)
    if (inliers[(size_t)i]) vbInliers[mvKeyPointIndices[(size_t)i]] = true;
  cv::Mat Tcw(4, 4, cv::CV_32F);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) Tcw.at<float>(r, c) = r < 3 ? (c < 3 ? q.Tcw[3 * r + c] : q.Tcw[9 + r]) : (c == 3 ? 1.0f : 0.0f);
  return Tcw;
}

// ------------------------------------------------------------------------------------------------ Sim3Solver (src/Sim3Solver.cpp)
extern "C" int hm_sim3_iterate_host(int F, int njobs, cms_sim3_job* jobs);      // sim3_host.cpp: the host build of csrc/cms_sim3_core.h

Sim3Solver::Sim3Solver(const Sim3KeyFrameView& pKF1, const Sim3KeyFrameView& pKF2, const std::vector<int>& vpMatched12, const bool bFixScale) : mbFixScale(bFixScale) {
  const std::vector<int>& vpKeyFrameMP1 = pKF1.mvpMapPointMatches;
  mN1 = (int)vpMatched12.size();
  const int F = CamModelGeneral::GetCamera()->GetCubeFaceWidth();
  for (int i1 = 0; i1 < mN1; i1++) {      // :66-127
    if (vpMatched12[i1] < 0) continue;
    if (i1 >= (int)vpKeyFrameMP1.size() || vpKeyFrameMP1[i1] < 0) continue;      // !pMP1
    const Sim3MapPointView& pMP1 = pKF1.mvMapPoints[(size_t)vpKeyFrameMP1[i1]];
    const Sim3MapPointView& pMP2 = pKF2.mvMapPoints[(size_t)vpMatched12[i1]];
    if (pMP1.mbBad || pMP2.mbBad) continue;
    const int indexKF1 = pMP1.mnIndexInKeyFrame, indexKF2 = pMP2.mnIndexInKeyFrame;
    if (indexKF1 < 0 || indexKF2 < 0) continue;
    cv::Vec3f X3D1c, X3D2c;
    float u, v;
    for (int r = 0; r < 3; ++r) X3D1c(r) = cms_sim3_row(pKF1.Rcw + 3 * r, pMP1.mWorldPos(0), pMP1.mWorldPos(1), pMP1.mWorldPos(2), pKF1.tcw[r]);
    track_rays_to_cubemap(F, X3D1c(0), X3D1c(1), X3D1c(2), u, v);
    if (u < 0 || v < 0) continue;
    for (int r = 0; r < 3; ++r) X3D2c(r) = cms_sim3_row(pKF2.Rcw + 3 * r, pMP2.mWorldPos(0), pMP2.mWorldPos(1), pMP2.mWorldPos(2), pKF2.tcw[r]);
    track_rays_to_cubemap(F, X3D2c(0), X3D2c(1), X3D2c(2), u, v);
    if (u < 0 || v < 0) continue;
    mvX3Dc1.push_back(X3D1c);
    mvX3Dc2.push_back(X3D2c);
    const float sigmaSquare1 = pKF1.mvLevelSigma2[(size_t)pKF1.mvKeyOctaves[(size_t)indexKF1]];
    const float sigmaSquare2 = pKF2.mvLevelSigma2[(size_t)pKF2.mvKeyOctaves[(size_t)indexKF2]];
    mvnMaxError1.push_back(9.210 * sigmaSquare1);
    mvnMaxError2.push_back(9.210 * sigmaSquare2);
    mvnIndices1.push_back((size_t)i1);
  }
  draw = [](int min, int max) { const int d = max - min + 1; return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min; };
  SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
  mRansacProb = probability;
  mRansacMinInliers = minInliers;
  N = (int)mvX3Dc1.size();
  if (cms_sim3_ransac_parameters(N, probability, minInliers, maxIterations, &mRansacMaxIts))
    throw std::runtime_error(std::string("cms_sim3_ransac_parameters: ") + cms_last_error());
  mnIterations = 0;
  mvbBestInliers.resize((size_t)N + 1, 0);
}

cv::Mat Sim3Solver::find(std::vector<bool>& vbInliers12, int& nInliers) {
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  bNoMore = false; vbInliers = std::vector<bool>((size_t)mN1, false); nInliers = 0;
  if (N < mRansacMinInliers) { bNoMore = true; return cv::Mat(); }      // :170-174
  if (mRansacMinInliers < 3) throw std::runtime_error("Sim3Solver::iterate: minInliers below the three pairs of a hypothesis");
  const int H = std::max(std::max(mRansacMaxIts - mnIterations, nIterations), 0);
  std::vector<int> draws((size_t)H * 3);
  for (int i = 0; i < H; ++i)
    for (int k = 0; k < 3; ++k) draws[(size_t)i * 3 + k] = draw(0, N - k - 1);      // RandomInt(0, vAvailableIndices.size()-1), :192
  std::vector<uint8_t> inliers((size_t)N + 1, 0);
  cms_sim3_job q = {};
  q.N = N; q.x3dc1 = N ? &mvX3Dc1[0](0) : nullptr; q.x3dc2 = N ? &mvX3Dc2[0](0) : nullptr; q.max_err1 = mvnMaxError1.data(); q.max_err2 = mvnMaxError2.data();
  q.fix_scale = mbFixScale ? 1 : 0; q.min_inliers = mRansacMinInliers; q.max_its = mRansacMaxIts; q.n_iterations = nIterations;
  q.n_draws = (int)draws.size(); q.draws = draws.data();
  q.iterations = mnIterations; q.best_inliers = mnBestInliers; q.best_mask = mvbBestInliers.data(); q.inliers = inliers.data();
  std::memcpy(q.best_R, mBestRotation, sizeof(mBestRotation)); std::memcpy(q.best_t, mBestTranslation, sizeof(mBestTranslation));
  std::memcpy(&q.best_s, &mBestScale, sizeof(float)); std::memcpy(q.best_T12, mBestT12, sizeof(mBestT12));
  if (engine == HOST_CORE) {
    const int rc = hm_sim3_iterate_host(CamModelGeneral::GetCamera()->GetCubeFaceWidth(), 1, &q);
    if (rc) throw std::runtime_error("Sim3Solver::iterate: the job was refused (" + std::to_string(rc) + ")");
  } else {
    cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures > 0 ? g_ctx_orb.nfeatures : 1000, g_ctx_orb.nfeatures > 0 ? g_ctx_orb.scale_factor : 1.2f,
                                 g_ctx_orb.nfeatures > 0 ? g_ctx_orb.nlevels : 8, g_ctx_orb.nfeatures > 0 ? g_ctx_orb.ini_th_fast : 20,
                                 g_ctx_orb.nfeatures > 0 ? g_ctx_orb.min_th_fast : 7);
    cms_sim3* h = nullptr;
    if (cms_sim3_create(&h, 0, 1, std::max(N, 1), std::max(H, 1))) throw std::runtime_error(std::string("cms_sim3_create: ") + cms_last_error());
    const int rc = cms_sim3_iterate(h, ctx, 1, &q);
    cms_sim3_destroy(h);
    if (rc) throw std::runtime_error(std::string("cms_sim3_iterate: ") + cms_last_error());
  }
  mnIterations = q.iterations; mnBestInliers = q.best_inliers;
  std::memcpy(mBestRotation, q.best_R, sizeof(mBestRotation)); std::memcpy(mBestTranslation, q.best_t, sizeof(mBestTranslation));
  std::memcpy(&mBestScale, &q.best_s, sizeof(float)); std::memcpy(mBestT12, q.best_T12, sizeof(mBestT12));
  bNoMore = q.no_more != 0;
  if (q.status == 0) return cv::Mat();
  nInliers = q.n_inliers;
  for (int i = 0; i < N; i++)      // :219-221
    if (inliers[(size_t)i]) vbInliers[mvnIndices1[(size_t)i]] = true;
  cv::Mat T12(4, 4, cv::CV_32F);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) T12.at<float>(r, c) = r < 3 ? q.T12[4 * r + c] : (c == 3 ? 1.0f : 0.0f);
  return T12;
}

cv::Mat Sim3Solver::GetEstimatedRotation() {
  cv::Mat R(3, 3, cv::CV_32F);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R.at<float>(r, c) = mBestRotation[3 * r + c];
  return R;
}
cv::Mat Sim3Solver::GetEstimatedTranslation() {
  cv::Mat t(3, 1, cv::CV_32F);
  for (int r = 0; r < 3; ++r) t.at<float>(r, 0) = mBestTranslation[r];
  return t;
}
float Sim3Solver::GetEstimatedScale() { return mBestScale; }

// ------------------------------------------------------------------------------------------------ Optimizer::OptimizeSim3 (src/Optimizer.cpp:888-1091)
extern "C" int hm_sim3_optimize_host(int F, int njobs, cms_sim3_opt_job* jobs);      // sim3_opt_host.cpp: the host build of csrc/cms_sim3_opt_core.h
extern "C" const char* hm_sim3_opt_last_reason();

Sim3OptGraph Optimizer::CollectSim3Graph(const Sim3OptKeyFrameView& pKF1, const Sim3OptKeyFrameView& pKF2, const std::vector<int>& vpMatches1) {
  Sim3OptGraph g;
  const int N = (int)vpMatches1.size();
  const std::vector<int>& vpMapPoints1 = pKF1.mvpMapPointMatches;
  for (int i = 0; i < N; i++) {      // :941-1028
    if (vpMatches1[i] < 0) continue;                                                     // !vpMatches1[i]
    if (i >= (int)vpMapPoints1.size() || vpMapPoints1[i] < 0) continue;                  // !pMP1
    const Sim3MapPointView& pMP1 = pKF1.mvMapPoints[(size_t)vpMapPoints1[i]];
    const Sim3MapPointView& pMP2 = pKF2.mvMapPoints[(size_t)vpMatches1[i]];
    const int i2 = pMP2.mnIndexInKeyFrame;                                               // pMP2->GetIndexInKeyFrame(pKF2)
    if (pMP1.mbBad || pMP2.mbBad || i2 < 0) continue;
    for (int r = 0; r < 3; ++r) g.x3dc1.push_back(cms_sim3_row(pKF1.Rcw + 3 * r, pMP1.mWorldPos(0), pMP1.mWorldPos(1), pMP1.mWorldPos(2), pKF1.tcw[r]));
    for (int r = 0; r < 3; ++r) g.x3dc2.push_back(cms_sim3_row(pKF2.Rcw + 3 * r, pMP2.mWorldPos(0), pMP2.mWorldPos(1), pMP2.mWorldPos(2), pKF2.tcw[r]));
    g.kp1.push_back(pKF1.mvKeyPts[(size_t)i].x); g.kp1.push_back(pKF1.mvKeyPts[(size_t)i].y);
    g.kp2.push_back(pKF2.mvKeyPts[(size_t)i2].x); g.kp2.push_back(pKF2.mvKeyPts[(size_t)i2].y);
    g.invSigma2_1.push_back(pKF1.mvInvLevelSigma2[(size_t)pKF1.mvKeyOctaves[(size_t)i]]);
    g.invSigma2_2.push_back(pKF2.mvInvLevelSigma2[(size_t)pKF2.mvKeyOctaves[(size_t)i2]]);
    g.vnIndexEdge.push_back((size_t)i);
  }
  return g;
}

int Optimizer::OptimizeSim3(const Sim3OptKeyFrameView& pKF1, const Sim3OptKeyFrameView& pKF2, std::vector<int>& vpMatches1, Sim3Value& g2oS12, const float th2,
                            const bool bFixScale, Engine engine, int jacobian) {
  Sim3OptGraph g = CollectSim3Graph(pKF1, pKF2, vpMatches1);
  const int n = (int)g.vnIndexEdge.size();
  std::vector<uint8_t> keep((size_t)n + 1, 1);
  for (std::vector<float>* v : {&g.x3dc1, &g.x3dc2, &g.kp1, &g.kp2, &g.invSigma2_1, &g.invSigma2_2}) v->push_back(0.0f);      // (never empty: data() stays valid)
  cms_sim3_opt_job q = {};
  q.N = n; q.x3dc1 = g.x3dc1.data(); q.x3dc2 = g.x3dc2.data(); q.kp1 = g.kp1.data(); q.kp2 = g.kp2.data(); q.inv_sigma2_1 = g.invSigma2_1.data(); q.inv_sigma2_2 = g.invSigma2_2.data();
  std::memcpy(q.R12, g2oS12.R, sizeof(q.R12)); std::memcpy(q.t12, g2oS12.t, sizeof(q.t12)); q.s12 = g2oS12.s;
  q.th2 = th2; q.fix_scale = bFixScale ? 1 : 0; q.jacobian = jacobian; q.keep = keep.data();
  if (engine == HOST_CORE) {
    const int rc = hm_sim3_optimize_host(CamModelGeneral::GetCamera()->GetCubeFaceWidth(), 1, &q);
    if (rc) throw std::runtime_error(std::string("Optimizer::OptimizeSim3: the job was refused: ") + hm_sim3_opt_last_reason());
  } else {
    cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures > 0 ? g_ctx_orb.nfeatures : 1000, g_ctx_orb.nfeatures > 0 ? g_ctx_orb.scale_factor : 1.2f,
                                 g_ctx_orb.nfeatures > 0 ? g_ctx_orb.nlevels : 8, g_ctx_orb.nfeatures > 0 ? g_ctx_orb.ini_th_fast : 20,
                                 g_ctx_orb.nfeatures > 0 ? g_ctx_orb.min_th_fast : 7);
    cms_sim3_opt* h = nullptr;
    if (cms_sim3_opt_create(&h, 0, 1, std::max(n, 1))) throw std::runtime_error(std::string("cms_sim3_opt_create: ") + cms_last_error());
    const int rc = cms_sim3_optimize(h, ctx, 1, &q);
    cms_sim3_opt_destroy(h);
    if (rc) throw std::runtime_error(std::string("cms_sim3_optimize: ") + cms_last_error());
  }
  for (int k = 0; k < n; ++k)
    if (!keep[(size_t)k]) vpMatches1[g.vnIndexEdge[(size_t)k]] = -1;      // vpMatches1[idx] = NULL (:1046, :1080)
  std::memcpy(g2oS12.q, q.q12, sizeof(g2oS12.q)); std::memcpy(g2oS12.t, q.t12_out, sizeof(g2oS12.t)); g2oS12.s = q.s12_out;
  return q.n_inliers;
}

// ------------------------------------------------------------------------------------------------ Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:623-886)
extern "C" int hm_essential_graph_optimize_host(int njobs, cms_ess_graph_job* jobs);      // ess_graph_host.cpp: the host build of csrc/cms_ess_graph_core.h
extern "C" int hm_sim3_correct_points_host(int n, const float* pos_in, const int* ref, int K, const double* S_old, const double* S_new, float* pos_out);
extern "C" const char* hm_ess_graph_last_reason();

EssGraph Optimizer::CollectEssentialGraph(const EssentialGraphMap& pMap, int pLoopKF, int pCurKF, const KeyFrameAndPose& NonCorrectedSim3,
                                          const KeyFrameAndPose& CorrectedSim3, const std::map<int, std::set<int>>& LoopConnections) {
  const std::vector<EssGraphKeyFrameView>& vpKFs = pMap.mvpKeyFrames;
  const int nKF = (int)vpKFs.size();
  const int minFeat = 100;
  EssGraph g;
  // :650-686: the vertices.  g2o indexes them by mnId; here they are compacted in mnId order, bad key frames left out
  for (int i = 0; i < nKF; i++)
    if (!vpKFs[(size_t)i].mbBad) g.vertexKF.push_back(i);
  std::sort(g.vertexKF.begin(), g.vertexKF.end(), [&](int a, int b) { return vpKFs[(size_t)a].mnId < vpKFs[(size_t)b].mnId; });
  std::vector<int> vertexOf((size_t)nKF, -1);
  for (size_t v = 0; v < g.vertexKF.size(); ++v) vertexOf[(size_t)g.vertexKF[v]] = (int)v;
  auto put = [](std::vector<double>& dst, const Sim3Pose& S) { dst.insert(dst.end(), S.q, S.q + 4); dst.insert(dst.end(), S.t, S.t + 3); dst.push_back(S.s); };
  for (int kf : g.vertexKF) {
    const EssGraphKeyFrameView& pKF = vpKFs[(size_t)kf];
    Sim3Pose Siw;
    KeyFrameAndPose::const_iterator it = CorrectedSim3.find(kf);
    if (it != CorrectedSim3.end()) {
      Siw = it->second;
    } else {      // g2o::Sim3 Siw(Rcw, tcw, 1.0) of the float pose widened (Converter::toMatrix3d / toVector3d)
      double R[9], t[3];
      for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)pKF.Tcw[4 * r + c]; t[r] = (double)pKF.Tcw[4 * r + 3]; }
      CmsS3 S;
      cms_s3o_from_Rts(R, t, 1.0, &S);
      std::memcpy(Siw.q, S.q, sizeof(Siw.q)); std::memcpy(Siw.t, S.t, sizeof(Siw.t)); Siw.s = S.s;
    }
    put(g.Scw, Siw);
    KeyFrameAndPose::const_iterator itn = NonCorrectedSim3.find(kf);      // what :737-741, :755-760, :776-781 and :805-810 pick per edge end
    put(g.Snc, itn != NonCorrectedSim3.end() ? itn->second : Siw);
  }
  g.fixed = pLoopKF >= 0 && pLoopKF < nKF ? vertexOf[(size_t)pLoopKF] : -1;
  auto weight = [&](const EssGraphKeyFrameView& k, int other) {      // KeyFrame::GetWeight
    for (size_t c = 0; c < k.mvpOrderedConnectedKeyFrames.size(); ++c)
      if (k.mvpOrderedConnectedKeyFrames[c] == other) return k.mvOrderedWeights[c];
    return 0;
  };
  auto add = [&](int kfi, int kfj, int kind) {
    if (kfj < 0 || kfj >= nKF || vertexOf[(size_t)kfi] < 0 || vertexOf[(size_t)kfj] < 0) return false;
    g.edges.push_back(vertexOf[(size_t)kfi]); g.edges.push_back(vertexOf[(size_t)kfj]); g.edges.push_back(kind);
    return true;
  };
  std::set<std::pair<long unsigned int, long unsigned int>> sInsertedEdges;
  // :693-722: loop-connection edges, measured from vScw
  for (std::map<int, std::set<int>>::const_iterator mit = LoopConnections.begin(); mit != LoopConnections.end(); ++mit) {
    if (mit->first < 0 || mit->first >= nKF) continue;
    const EssGraphKeyFrameView& pKF = vpKFs[(size_t)mit->first];
    const long unsigned int nIDi = pKF.mnId;
    for (int other : mit->second) {
      if (other < 0 || other >= nKF) continue;
      const long unsigned int nIDj = vpKFs[(size_t)other].mnId;
      if ((nIDi != vpKFs[(size_t)pCurKF].mnId || nIDj != vpKFs[(size_t)pLoopKF].mnId) && weight(pKF, other) < minFeat) continue;
      if (add(mit->first, other, 0)) sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }
  // :724-825: normal edges, measured from NonCorrectedSim3 where present
  for (int i = 0; i < nKF; i++) {
    const EssGraphKeyFrameView& pKF = vpKFs[(size_t)i];
    if (pKF.mbBad) continue;
    const int pParentKF = pKF.mpParent;
    if (pParentKF >= 0) add(i, pParentKF, 1);                                             // spanning tree edge
    for (int pLKF : pKF.mspLoopEdges)                                                     // loop edges
      if (pLKF >= 0 && pLKF < nKF && vpKFs[(size_t)pLKF].mnId < pKF.mnId) add(i, pLKF, 1);
    for (size_t c = 0; c < pKF.mvpOrderedConnectedKeyFrames.size(); ++c) {                 // covisibility graph edges: GetCovisiblesByWeight(minFeat)
      if (pKF.mvOrderedWeights[c] < minFeat) break;
      const int pKFn = pKF.mvpOrderedConnectedKeyFrames[c];
      if (pKFn < 0 || pKFn >= nKF || pKFn == pParentKF || pKF.mspChildrens.count(pKFn) || pKF.mspLoopEdges.count(pKFn)) continue;
      const EssGraphKeyFrameView& n = vpKFs[(size_t)pKFn];
      if (n.mbBad || !(n.mnId < pKF.mnId)) continue;
      if (sInsertedEdges.count(std::make_pair(std::min(pKF.mnId, n.mnId), std::max(pKF.mnId, n.mnId)))) continue;
      add(i, pKFn, 1);
    }
  }
  return g;
}

void Optimizer::OptimizeEssentialGraph(EssentialGraphMap& pMap, int pLoopKF, int pCurKF, const KeyFrameAndPose& NonCorrectedSim3, const KeyFrameAndPose& CorrectedSim3,
                                       const std::map<int, std::set<int>>& LoopConnections, const bool& bFixScale, Engine engine) {
  EssGraph g = CollectEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections);
  const int N = (int)g.vertexKF.size(), E = (int)g.edges.size() / 3;
  if (N == 0 || g.fixed < 0) throw std::runtime_error("Optimizer::OptimizeEssentialGraph: pLoopKF has no vertex");
  std::vector<double> S_out(8 * (size_t)N);
  std::vector<float> Tiw(12 * (size_t)N);
  g.edges.push_back(0);      // (never empty: data() stays valid)
  cms_ess_graph_job q = {};
  q.N = N; q.Scw = g.Scw.data(); q.Snc = g.Snc.data(); q.fixed = g.fixed; q.E = E; q.edges = g.edges.data(); q.fix_scale = bFixScale ? 1 : 0;
  q.iterations = 20; q.lambda_init = 1e-16; q.S_out = S_out.data(); q.Tiw_out = Tiw.data();
  // :854-885: the reference key frame of every map point, as a vertex
  std::vector<int> vertexOfId;
  for (int v = 0; v < N; ++v) {
    const size_t id = (size_t)pMap.mvpKeyFrames[(size_t)g.vertexKF[(size_t)v]].mnId;
    if (vertexOfId.size() <= id) vertexOfId.resize(id + 1, -1);
    vertexOfId[id] = v;
  }
  const size_t nMP = pMap.mvpMapPoints.size();
  std::vector<float> pos(3 * nMP + 3), pos_out(3 * nMP + 3);
  std::vector<int> ref(nMP + 1, -1);
  const long unsigned int curId = pMap.mvpKeyFrames[(size_t)pCurKF].mnId;
  for (size_t i = 0; i < nMP; ++i) {
    const EssGraphMapPointView& pMP = pMap.mvpMapPoints[i];
    std::memcpy(&pos[3 * i], pMP.mWorldPos, 12);
    if (pMP.mbBad) continue;
    size_t nIDr;
    if (pMP.mnCorrectedByKF == curId) nIDr = (size_t)pMP.mnCorrectedReference;
    else if (pMP.mpRefKF >= 0) nIDr = (size_t)pMap.mvpKeyFrames[(size_t)pMP.mpRefKF].mnId;
    else continue;
    ref[i] = nIDr < vertexOfId.size() ? vertexOfId[nIDr] : -1;
  }
  if (engine == HOST_CORE) {
    if (hm_essential_graph_optimize_host(1, &q)) throw std::runtime_error(std::string("Optimizer::OptimizeEssentialGraph: the job was refused: ") + hm_ess_graph_last_reason());
    if (hm_sim3_correct_points_host((int)nMP, pos.data(), ref.data(), N, g.Scw.data(), S_out.data(), pos_out.data()))
      throw std::runtime_error(std::string("Optimizer::OptimizeEssentialGraph: the points were refused: ") + hm_ess_graph_last_reason());
  } else {
    cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures > 0 ? g_ctx_orb.nfeatures : 1000, g_ctx_orb.nfeatures > 0 ? g_ctx_orb.scale_factor : 1.2f,
                                 g_ctx_orb.nfeatures > 0 ? g_ctx_orb.nlevels : 8, g_ctx_orb.nfeatures > 0 ? g_ctx_orb.ini_th_fast : 20,
                                 g_ctx_orb.nfeatures > 0 ? g_ctx_orb.min_th_fast : 7);
    std::vector<int> first;
    const long long blocks = cms_eg_envelope(N, g.fixed, E, g.edges.data(), first);
    if (blocks > 0x7fffffffLL) throw std::runtime_error("Optimizer::OptimizeEssentialGraph: the envelope is too large");
    cms_ess_graph* h = nullptr;
    if (cms_ess_graph_create(&h, 0, 1, N, std::max(E, 1), (int)std::max(blocks, 1LL))) throw std::runtime_error(std::string("cms_ess_graph_create: ") + cms_last_error());
    const int rc = cms_essential_graph_optimize(h, ctx, 1, &q);
    cms_ess_graph_destroy(h);
    if (rc) throw std::runtime_error(std::string("cms_essential_graph_optimize: ") + cms_last_error());
    if (cms_sim3_correct_points(ctx, (int)nMP, pos.data(), ref.data(), N, g.Scw.data(), S_out.data(), pos_out.data()))
      throw std::runtime_error(std::string("cms_sim3_correct_points: ") + cms_last_error());
  }
  for (int v = 0; v < N; ++v) std::memcpy(pMap.mvpKeyFrames[(size_t)g.vertexKF[(size_t)v]].Tcw, &Tiw[12 * (size_t)v], 48);      // pKFi->SetPose(Tiw)
  for (size_t i = 0; i < nMP; ++i)
    if (ref[i] >= 0) std::memcpy(pMap.mvpMapPoints[i].mWorldPos, &pos_out[3 * i], 12);                                          // pMP->SetWorldPos
}

// ------------------------------------------------------------------------------------------------ Initializer (src/Initializer.cpp)
extern "C" int hm_init_two_view_host(int F, float cos_fov, int njobs, cms_init_job* jobs);      // init_host.cpp: the host build of csrc/cms_init_core.h

Initializer::Initializer(const FrameView& ReferenceFrame, float sigma, int iterations) {
  mvKeys1 = ReferenceFrame.mvKeys;
  mvKeyRays1 = ReferenceFrame.mvKeyRays;
  mSigma = sigma;
  mSigma2 = sigma * sigma;
  mMaxIterations = iterations;
  draw = [](int min, int max) {
    static const bool seeded = (srand(0), true);      // DUtils::Random::SeedRandOnce(0), :90
    (void)seeded;
    const int d = max - min + 1;
    return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
  };
}

bool Initializer::InitializeWithRays(const FrameView& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
                                     std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
  mvKeys2 = CurrentFrame.mvKeys;
  mvKeyRays2 = CurrentFrame.mvKeyRays;
  mvMatches12.clear();
  mvMatches12.reserve(mvKeys2.size());
  mvbMatched1.resize(mvKeys1.size());
  for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {      // :64-73
    if (vMatches12[i] >= 0) {
      mvMatches12.push_back(std::make_pair((int)i, vMatches12[i]));
      mvbMatched1[i] = true;
    } else
      mvbMatched1[i] = false;
  }
  const int N = (int)mvMatches12.size();
  R21 = cv::Mat(); t21 = cv::Mat();
  mnBestIteration = -1; mnInliers = 0; mnWinner = -1; mfScore = 0;
  for (int h = 0; h < 4; ++h) { mnGood[h] = 0; mfParallax[h] = 0; }
  if (N < 8 || mMaxIterations < 1 || vMatches12.size() != mvKeys1.size()) return false;
  std::vector<size_t> vAllIndices, vAvailableIndices;
  vAllIndices.reserve(N);
  for (int i = 0; i < N; i++) vAllIndices.push_back(i);
  mvSets = std::vector<std::vector<size_t>>(mMaxIterations, std::vector<size_t>(8, 0));
  std::vector<int> draws((size_t)mMaxIterations * 8);
  for (int it = 0; it < mMaxIterations; it++) {      // :92-107
    vAvailableIndices = vAllIndices;
    for (size_t j = 0; j < 8; j++) {
      const int randi = draw(0, (int)vAvailableIndices.size() - 1);
      draws[(size_t)it * 8 + j] = randi;
      mvSets[it][j] = vAvailableIndices[randi];
      vAvailableIndices[randi] = vAvailableIndices.back();
      vAvailableIndices.pop_back();
    }
  }
  const size_t n1 = mvKeys1.size(), n2 = mvKeys2.size();
  std::vector<float> keys1(2 * n1), keys2(2 * n2), p3d(3 * n1);
  std::vector<uint8_t> tri(n1);
  for (size_t i = 0; i < n1; ++i) { keys1[2 * i] = mvKeys1[i].pt.x; keys1[2 * i + 1] = mvKeys1[i].pt.y; }
  for (size_t i = 0; i < n2; ++i) { keys2[2 * i] = mvKeys2[i].pt.x; keys2[2 * i + 1] = mvKeys2[i].pt.y; }
  cms_init_job q = {};
  q.n1 = (int)n1; q.n2 = (int)n2; q.keys1 = keys1.data(); q.rays1 = &mvKeyRays1[0](0); q.keys2 = keys2.data(); q.rays2 = n2 ? &mvKeyRays2[0](0) : nullptr;
  q.matches12 = vMatches12.data(); q.sigma = mSigma; q.iterations = mMaxIterations; q.n_draws = (int)draws.size(); q.draws = draws.data();
  q.p3d = p3d.data(); q.triangulated = tri.data();
  if (engine == HOST_CORE) {
    const int rc = hm_init_two_view_host(CamModelGeneral::GetCamera()->GetCubeFaceWidth(), CamModelGeneral::GetCamera()->GetCosFovTh(), 1, &q);
    if (rc) throw std::runtime_error("Initializer::InitializeWithRays: the job was refused (" + std::to_string(rc) + ")");
  } else {
    cms_ctx* ctx = SharedContext(g_ctx_orb.nfeatures > 0 ? g_ctx_orb.nfeatures : 1000, g_ctx_orb.nfeatures > 0 ? g_ctx_orb.scale_factor : 1.2f,
                                 g_ctx_orb.nfeatures > 0 ? g_ctx_orb.nlevels : 8, g_ctx_orb.nfeatures > 0 ? g_ctx_orb.ini_th_fast : 20,
                                 g_ctx_orb.nfeatures > 0 ? g_ctx_orb.min_th_fast : 7);
    cms_init* h = nullptr;
    if (cms_init_create(0, 1, N, (int)n1, mMaxIterations, &h)) throw std::runtime_error(std::string("cms_init_create: ") + cms_last_error());
    const int rc = cms_init_two_view(h, ctx, 1, &q);
    cms_init_destroy(h);
    if (rc) throw std::runtime_error(std::string("cms_init_two_view: ") + cms_last_error());
  }
  mnBestIteration = q.best_iteration; mnInliers = q.n_inliers; mnWinner = q.winner; mfScore = q.score;
  for (int h = 0; h < 4; ++h) { mnGood[h] = q.nGood[h]; mfParallax[h] = q.parallax[h]; }
  if (q.status != 1) return false;
  vP3D.resize(n1);
  vbTriangulated = std::vector<bool>(n1, false);
  for (size_t i = 0; i < n1; ++i) {
    vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
    vbTriangulated[i] = tri[i] != 0;
  }
  R21 = cv::Mat(3, 3, cv::CV_32F); t21 = cv::Mat(3, 1, cv::CV_32F);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R21.at<float>(r, c) = q.R21[3 * r + c];
    t21.at<float>(r, 0) = q.t21[r];
  }
  return true;
}

// ---- ORBVocabulary (DBoW2::TemplatedVocabulary) and Frame / KeyFrame::ComputeBoW
struct ORBVocabulary::Impl {
  VocabularyText text;
  CmsVocabTree tree;
  bool loaded = false;
  cms_vocab* dev = nullptr;
};
ORBVocabulary::ORBVocabulary() : impl_(new Impl()) {}
ORBVocabulary::~ORBVocabulary() {
  if (impl_->dev) cms_vocab_destroy(impl_->dev);
  delete impl_;
}
bool ORBVocabulary::setTree(const VocabularyText& t) {
  CmsVocabTree tree;
  const char* why = cms_vocab_relayout(t.k, t.L, t.scoring, t.weighting, t.nodes(), t.parent.data(), t.is_leaf.data(), t.desc.data(), t.weight.data(), &tree);
  if (why) { error_ = why; return false; }
  if (impl_->dev) { cms_vocab_destroy(impl_->dev); impl_->dev = nullptr; }
  impl_->text = t; impl_->tree = std::move(tree); impl_->loaded = true;
  error_.clear();
  return true;
}
bool ORBVocabulary::loadFromTextFile(const std::string& filename) {
  VocabularyText t;
  if (!LoadVocabularyText(filename, &t, &error_)) return false;
  return setTree(t);
}
void ORBVocabulary::saveToTextFile(const std::string& filename) const {
  std::ofstream f(filename.c_str(), std::ios::binary);
  f << FormatVocabularyText(impl_->text);
}
bool ORBVocabulary::empty() const { return !impl_->loaded || impl_->tree.n_words == 0; }
unsigned ORBVocabulary::size() const { return impl_->loaded ? (unsigned)impl_->tree.n_words : 0u; }
const VocabularyText& ORBVocabulary::tree() const { return impl_->text; }
cms_vocab* ORBVocabulary::deviceHandle() const {
  if (empty()) throw std::runtime_error("ORBVocabulary: empty vocabulary");
  if (!impl_->dev) {
    const VocabularyText& t = impl_->text;
    if (cms_vocab_create(&impl_->dev, kSharedDevice, t.k, t.L, t.scoring, t.weighting, t.nodes(), t.parent.data(), t.is_leaf.data(), t.desc.data(), t.weight.data()) != CMS_OK)
      throw std::runtime_error(std::string("cms_vocab_create failed: ") + cms_last_error());
  }
  return impl_->dev;
}
void ORBVocabulary::transform(const std::vector<cv::Mat>& features, BowVector& v, FeatureVector& fv, int levelsup) const {
  v.clear();
  fv.clear();
  if (empty()) return;      // :1134
  const int n = (int)features.size();
  std::vector<uint8_t> desc(32 * (size_t)std::max(n, 1));
  for (int i = 0; i < n; ++i) std::memcpy(desc.data() + 32 * (size_t)i, features[(size_t)i].data, 32);
  CmsVocabResult r;
  if (engine == HOST_CORE) {
    cms_vocab_transform_host(impl_->tree.view(), n, desc.data(), levelsup, &r);
  } else {
    // the shared context as the extractor sized it, or System's default one when the vocabulary is the first to need it (System.cpp loads it first)
    cms_ctx* ctx = g_ctx_orb.nfeatures > 0 ? SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast)
                                           : SharedContext(2000, 1.2f, 8, 20, 7);
    cms_vocab* dev = deviceHandle();
    const size_t cap = (size_t)std::max(n, 1);
    r.word_id.resize(cap); r.word_val.resize(cap); r.node_id.resize(cap); r.node_off.resize(cap + 1); r.node_feat.resize(cap);
    int nwords = 0, nnodes = 0;
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (cms_vocab_transform(dev, ctx, n, desc.data(), levelsup, &nwords, r.word_id.data(), r.word_val.data(), &nnodes, r.node_id.data(), r.node_off.data(),
                            r.node_feat.data()) != CMS_OK)
      throw std::runtime_error(std::string("cms_vocab_transform failed: ") + cms_last_error());
    r.word_id.resize((size_t)nwords); r.word_val.resize((size_t)nwords); r.node_id.resize((size_t)nnodes); r.node_off.resize((size_t)nnodes + 1);
  }
  for (size_t i = 0; i < r.word_id.size(); ++i) v.push_back(std::make_pair((unsigned)r.word_id[i], r.word_val[i]));
  for (size_t e = 0; e < r.node_id.size(); ++e)
    fv.push_back(std::make_pair((unsigned)r.node_id[e], std::vector<unsigned>(r.node_feat.begin() + r.node_off[e], r.node_feat.begin() + r.node_off[e + 1])));
}
// L1Scoring::score (ScoringObject.cpp:23-68); lower_bound on a map is the first entry with an id not smaller
double ORBVocabulary::score(const BowVector& v1, const BowVector& v2) const {
  if (impl_->loaded && impl_->text.scoring != CMS_VOC_L1_NORM) throw std::runtime_error("ORBVocabulary::score: only L1 scoring is supported");
  size_t i = 0, j = 0;
  double score = 0;
  while (i < v1.size() && j < v2.size()) {
    const double vi = v1[i].second, wi = v2[j].second;
    if (v1[i].first == v2[j].first) {
      score += fabs(vi - wi) - fabs(vi) - fabs(wi);
      ++i; ++j;
    } else if (v1[i].first < v2[j].first) {
      while (i < v1.size() && v1[i].first < v2[j].first) ++i;
    } else {
      while (j < v2.size() && v2[j].first < v1[i].first) ++j;
    }
  }
  score = -score / 2.0;
  return score;
}
// one 1 x 32 header per descriptor row (what Converter::toDescriptorVector hands to transform)
static std::vector<cv::Mat> descriptor_rows(const cv::Mat& m) {
  std::vector<cv::Mat> rows((size_t)std::max(m.rows, 0));
  for (size_t r = 0; r < rows.size(); ++r) rows[r] = m.row((int)r);
  return rows;
}
void FrameView::ComputeBoW(const ORBVocabulary& voc) {
  if (mBowVec.empty()) voc.transform(descriptor_rows(mDescriptors), mBowVec, mFeatVec, 4);
}
void KeyFrameView::ComputeBoW(const ORBVocabulary& voc) {
  if (mBowVec.empty() || mFeatVec.empty()) voc.transform(descriptor_rows(mDescriptors), mBowVec, mFeatVec, 4);
}


// ---- KeyFrameDatabase (src/KeyFrameDatabase.cpp)
struct KeyFrameDatabase::Impl {
  const ORBVocabulary* voc;
  int max_keyframes, max_features;
  CmsKfdbHost host;                          // HOST_CORE; also the slot table of both engines (which slot holds which view)
  std::map<KeyFrameView*, int> slot_of;      // key frames in the database
  std::vector<KeyFrameView*> kf_of;
  cms_kfstore* store = nullptr;              // DEVICE, made by the first add
  Impl(const ORBVocabulary& v, int K, int Fq) : voc(&v), max_keyframes(K), max_features(Fq), host(K, Fq), kf_of((size_t)K, nullptr) {}
  cms_ctx* ctx() const {
    return g_ctx_orb.nfeatures > 0 ? SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast)
                                   : SharedContext(2000, 1.2f, 8, 20, 7);
  }
  void need_l1() const {
    if (!voc->empty() && voc->tree().scoring != CMS_VOC_L1_NORM) throw std::runtime_error("KeyFrameDatabase: only L1 scoring is supported");
  }
  std::vector<KeyFrameView*> detect(Engine engine, int mode, const BowVector& bow, float min_score, const std::vector<KeyFrameView*>& connected) {
    need_l1();
    std::vector<int> ids(bow.size() + 1), conn;
    std::vector<double> vals(bow.size() + 1);
    for (size_t i = 0; i < bow.size(); ++i) { ids[i] = (int)bow[i].first; vals[i] = bow[i].second; }
    for (KeyFrameView* c : connected) { auto it = slot_of.find(c); if (it != slot_of.end()) conn.push_back(it->second); }
    std::vector<int> cand;
    if (engine == HOST_CORE) {
      CmsKfdbQuery q;
      q.mode = mode; q.group = 0; q.bow = CmsKfdbBow{(int)bow.size(), ids.data(), vals.data()}; q.min_score = min_score; q.n_connected = (int)conn.size(); q.connected = conn.data();
      host.detect(q, &cand, nullptr, nullptr);
    } else if (store) {
      cms_kfdb_job j = {};
      j.mode = mode; j.group = 0; j.query = CMS_KFDB_QUERY_WORDS; j.nwords = (int)bow.size(); j.word_id = ids.data(); j.word_val = vals.data();
      j.min_score = min_score; j.n_connected = (int)conn.size(); j.connected = conn.data();
      cand.resize((size_t)max_keyframes);
      int n = 0;
      cms_ctx* c = ctx();
      std::lock_guard<std::mutex> lock(g_ctx_mutex);
      if (cms_kfdb_detect(store, c, 1, &j, max_keyframes, cand.data(), &n, nullptr, nullptr) != CMS_OK)
        throw std::runtime_error(std::string("cms_kfdb_detect failed: ") + cms_last_error());
      cand.resize((size_t)n);
    }
    std::vector<KeyFrameView*> out;
    for (int s : cand) out.push_back(kf_of[(size_t)s]);
    return out;
  }
};
KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary& voc, int max_keyframes, int max_features) : impl_(new Impl(voc, max_keyframes, max_features)) {}
KeyFrameDatabase::~KeyFrameDatabase() {
  if (impl_->store) cms_kfstore_destroy(impl_->store);
  delete impl_;
}
void KeyFrameDatabase::add(KeyFrameView* pKF) {
  Impl& m = *impl_;
  if (!pKF || m.slot_of.count(pKF)) throw std::runtime_error("KeyFrameDatabase::add: null key frame, or one that is in the database already");
  int slot = 0;
  while (slot < m.max_keyframes && m.kf_of[(size_t)slot]) ++slot;
  if (slot == m.max_keyframes) throw std::runtime_error("KeyFrameDatabase::add: more key frames than max_keyframes");
  const size_t n = pKF->mBowVec.size();
  std::vector<int> ids(n + 1);
  std::vector<double> vals(n + 1);
  for (size_t i = 0; i < n; ++i) { ids[i] = (int)pKF->mBowVec[i].first; vals[i] = pKF->mBowVec[i].second; }
  const int group = 0;
  m.host.refill(slot);
  if (m.host.set_bow(slot, (int)n, ids.data(), vals.data())) throw std::runtime_error("KeyFrameDatabase::add: the BowVector does not ascend or has more words than max_features");
  if (engine == DEVICE) {
    cms_ctx* c = m.ctx();
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!m.store && cms_kfstore_create(&m.store, c, m.max_keyframes, m.max_features, m.max_features) != CMS_OK)
      throw std::runtime_error(std::string("cms_kfstore_create failed: ") + cms_last_error());
    KfPack pack;
    const cms_keyframe k = pack_keyframe(*pKF, pack);
    if (cms_kfstore_put(m.store, slot, &k) != CMS_OK || cms_kfstore_set_bow(m.store, slot, (int)n, ids.data(), vals.data()) != CMS_OK ||
        cms_kfdb_add(m.store, 1, &slot, &group) != CMS_OK)
      throw std::runtime_error(std::string("KeyFrameDatabase::add failed: ") + cms_last_error());
  }
  m.host.add(1, &slot, &group);
  m.slot_of[pKF] = slot; m.kf_of[(size_t)slot] = pKF;
}
void KeyFrameDatabase::erase(KeyFrameView* pKF) {
  Impl& m = *impl_;
  auto it = m.slot_of.find(pKF);
  if (it == m.slot_of.end()) return;
  const int slot = it->second;
  m.host.erase(1, &slot);
  if (m.store && cms_kfdb_erase(m.store, 1, &slot) != CMS_OK) throw std::runtime_error(std::string("cms_kfdb_erase failed: ") + cms_last_error());
  m.kf_of[(size_t)slot] = nullptr;
  m.slot_of.erase(it);
}
void KeyFrameDatabase::clear() {
  Impl& m = *impl_;
  m.host.clear(-1);
  if (m.store && cms_kfdb_clear(m.store, -1) != CMS_OK) throw std::runtime_error(std::string("cms_kfdb_clear failed: ") + cms_last_error());
  m.slot_of.clear();
  std::fill(m.kf_of.begin(), m.kf_of.end(), nullptr);
}
void KeyFrameDatabase::SetBestCovisibilityKeyFrames(KeyFrameView* pKF, const std::vector<KeyFrameView*>& best) {
  Impl& m = *impl_;
  auto it = m.slot_of.find(pKF);
  if (it == m.slot_of.end()) throw std::runtime_error("KeyFrameDatabase::SetBestCovisibilityKeyFrames: the key frame is not in the database");
  int neigh[CMS_KFDB_COVIS];
  std::fill(neigh, neigh + CMS_KFDB_COVIS, -1);
  int n = 0;
  for (KeyFrameView* b : best) {      // (a covisible outside the database contributes nothing: it keeps no place)
    auto jt = m.slot_of.find(b);
    if (n < CMS_KFDB_COVIS && jt != m.slot_of.end()) neigh[n++] = jt->second;
  }
  const int slot = it->second;
  m.host.set_covisibles(1, &slot, neigh);
  if (m.store && cms_kfdb_set_covisibles(m.store, 1, &slot, neigh) != CMS_OK) throw std::runtime_error(std::string("cms_kfdb_set_covisibles failed: ") + cms_last_error());
}
std::vector<KeyFrameView*> KeyFrameDatabase::DetectRelocalizationCandidates(FrameView* F) {
  return impl_->detect(engine, CMS_KFDB_RELOC, F->mBowVec, 0.0f, std::vector<KeyFrameView*>());
}
std::vector<KeyFrameView*> KeyFrameDatabase::DetectLoopCandidates(KeyFrameView* pKF, float minScore, const std::vector<KeyFrameView*>& connected) {
  return impl_->detect(engine, CMS_KFDB_LOOP, pKF->mBowVec, minScore, connected);
}

// ---- Covisibility (src/KeyFrame.cpp:315-404, src/LocalMapping.cpp:561-619, src/Tracking.cpp:855-928)
struct Covisibility::Impl {
  Engine engine;
  int max_keyframes, max_features;
  CmsCovisHostStore host;                    // HOST_CORE
  cms_kfstore* store = nullptr;              // DEVICE, made by the first Build
  cms_covis* cv = nullptr;
  std::vector<KeyFrameView*> members;
  std::map<KeyFrameView*, int> pos_of;
  Impl(Engine e, int K, int Fq) : engine(e), max_keyframes(K), max_features(Fq), host(K, Fq, K) {}
  cms_ctx* ctx() const {
    return g_ctx_orb.nfeatures > 0 ? SharedContext(g_ctx_orb.nfeatures, g_ctx_orb.scale_factor, g_ctx_orb.nlevels, g_ctx_orb.ini_th_fast, g_ctx_orb.min_th_fast)
                                   : SharedContext(2000, 1.2f, 8, 20, 7);
  }
  int pos(KeyFrameView* k, const char* who) const {
    auto it = pos_of.find(k);
    if (it == pos_of.end()) throw std::runtime_error(std::string(who) + ": the key frame is not a member of the last Build");
    return it->second;
  }
  static void fail(const char* who) { throw std::runtime_error(std::string(who) + " failed: " + cms_last_error()); }
};
Covisibility::Covisibility(Engine engine, int max_keyframes, int max_features) : impl_(new Impl(engine, max_keyframes, max_features)) {}
Covisibility::~Covisibility() {
  if (impl_->cv) cms_covis_destroy(impl_->cv);
  if (impl_->store) cms_kfstore_destroy(impl_->store);
  delete impl_;
}
void Covisibility::Build(const std::vector<KeyFrameView*>& members) {
  Impl& m = *impl_;
  if ((int)members.size() > m.max_keyframes) throw std::runtime_error("Covisibility::Build: more key frames than max_keyframes");
  std::map<KeyFrameView*, int> pos_of;
  std::vector<int> slots(members.size() + 1);
  for (size_t i = 0; i < members.size(); ++i) {
    if (!members[i] || pos_of.count(members[i])) throw std::runtime_error("Covisibility::Build: a null key frame, or one listed twice");
    if ((int)members[i]->mvKeys.size() > m.max_features) throw std::runtime_error("Covisibility::Build: a key frame with more features than max_features");
    pos_of[members[i]] = (int)i; slots[i] = (int)i;
  }
  std::vector<std::vector<int>> rows(members.size());
  for (size_t i = 0; i < members.size(); ++i) {
    const KeyFrameView& k = *members[i];
    rows[i].resize(k.mvKeys.size() + 1);
    for (size_t f = 0; f < k.mvKeys.size(); ++f) {
      const bool bad = !k.mvbMapPointBad.empty() && k.mvbMapPointBad[f];
      rows[i][f] = (k.mvpMapPoints[f] >= 0 && !bad) ? (int)(k.mvpMapPoints[f] & 0x3FFFFFFF) : -1;
    }
  }
  if (m.engine == HOST_CORE) {
    for (size_t i = 0; i < members.size(); ++i) {
      std::vector<int> oct(members[i]->mvKeys.size() + 1);
      for (size_t f = 0; f < members[i]->mvKeys.size(); ++f) oct[f] = members[i]->mvKeys[f].octave;
      if (m.host.put((int)i, (int)members[i]->mvKeys.size(), rows[i].data(), oct.data())) throw std::runtime_error("Covisibility::Build: bad key frame");
    }
    if (m.host.build((int)members.size(), slots.data())) throw std::runtime_error("Covisibility::Build: a key frame names a map point twice");
  } else {
    cms_ctx* c = m.ctx();
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!m.store && cms_kfstore_create(&m.store, c, m.max_keyframes, m.max_features, m.max_features) != CMS_OK) Impl::fail("cms_kfstore_create");
    if (!m.cv && cms_covis_create(&m.cv, m.store, m.max_keyframes) != CMS_OK) Impl::fail("cms_covis_create");
    for (size_t i = 0; i < members.size(); ++i) {
      KfPack pack;
      cms_keyframe k = pack_keyframe(*members[i], pack);
      k.mp = rows[i].data();
      if (cms_kfstore_put(m.store, (int)i, &k) != CMS_OK) Impl::fail("cms_kfstore_put");
    }
    if (cms_covis_build(m.cv, (int)members.size(), slots.data()) != CMS_OK) Impl::fail("cms_covis_build");
  }
  m.members = members; m.pos_of.swap(pos_of);
}
Covisibility::Connections Covisibility::UpdateConnections(KeyFrameView* pKF, int th) {
  Impl& m = *impl_;
  const int job = m.pos(pKF, "Covisibility::UpdateConnections");
  const size_t M = m.members.size();
  std::vector<int> w(M), order(M);
  int n = 0;
  if (m.engine == HOST_CORE) {
    if (m.host.index.connections(1, &job, th, w.data(), order.data(), &n)) throw std::runtime_error("Covisibility::UpdateConnections: bad argument");
  } else {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (cms_covis_connections(m.cv, 1, &job, th, w.data(), order.data(), &n) != CMS_OK) Impl::fail("cms_covis_connections");
  }
  Connections out;
  for (size_t i = 0; i < M; ++i) if (w[i] > 0) out.weights[m.members[i]] = w[i];
  for (int i = 0; i < n; ++i) { out.ordered.push_back(m.members[(size_t)order[(size_t)i]]); out.orderedWeights.push_back(w[(size_t)order[(size_t)i]]); }
  return out;
}
std::vector<Covisibility::Culled> Covisibility::KeyFrameCulling(const std::vector<KeyFrameView*>& candidates, const std::vector<bool>& notErase, int thObs) {
  Impl& m = *impl_;
  const size_t Q = candidates.size();
  if (notErase.size() != Q) throw std::runtime_error("Covisibility::KeyFrameCulling: one mbNotErase per candidate");
  std::vector<int> jobs(Q + 1), nm(Q + 1), nr(Q + 1);
  std::vector<uint8_t> er(Q + 1), red(Q + 1);
  for (size_t i = 0; i < Q; ++i) { jobs[i] = m.pos(candidates[i], "Covisibility::KeyFrameCulling"); er[i] = notErase[i] ? 0 : 1; }
  const int off[2] = {0, (int)Q};
  if (m.engine == HOST_CORE) {
    if (m.host.index.culling(1, off, jobs.data(), er.data(), thObs, nm.data(), nr.data(), red.data())) throw std::runtime_error("Covisibility::KeyFrameCulling: a candidate listed twice");
  } else {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (cms_covis_culling(m.cv, 1, off, jobs.data(), er.data(), thObs, nm.data(), nr.data(), red.data()) != CMS_OK) Impl::fail("cms_covis_culling");
  }
  std::vector<Culled> out;
  for (size_t i = 0; i < Q; ++i) out.push_back(Culled{candidates[i], nm[i], nr[i], red[i] != 0});
  return out;
}
std::vector<KeyFrameView*> Covisibility::UpdateLocalKeyFrames(const std::vector<long>& framePoints, KeyFrameView** pKFmax, std::vector<int>* votes) {
  Impl& m = *impl_;
  const size_t M = m.members.size();
  std::vector<int> ids(framePoints.size() + 1), v(M + 1, 0);
  for (size_t i = 0; i < framePoints.size(); ++i) {
    if (framePoints[i] < 0) throw std::runtime_error("Covisibility::UpdateLocalKeyFrames: list the frame's map points, not its empty entries");
    ids[i] = (int)(framePoints[i] & 0x3FFFFFFF);
  }
  const int off[2] = {0, (int)framePoints.size()};
  if (m.engine == HOST_CORE) {
    if (m.host.index.votes(1, off, ids.data(), v.data())) throw std::runtime_error("Covisibility::UpdateLocalKeyFrames: bad argument");
  } else {
    cms_ctx* c = m.ctx();
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (cms_covis_votes(m.cv, c, 1, off, ids.data(), v.data()) != CMS_OK) Impl::fail("cms_covis_votes");
  }
  std::vector<KeyFrameView*> local;
  int max = 0;
  if (pKFmax) *pKFmax = nullptr;
  for (size_t i = 0; i < M; ++i) {      // Tracking.cpp:913-928: the map's order, a strict >
    if (v[i] == 0) continue;
    if (v[i] > max) { max = v[i]; if (pKFmax) *pKFmax = m.members[i]; }
    local.push_back(m.members[i]);
  }
  if (votes) votes->assign(v.begin(), v.begin() + (long)M);
  return local;
}
std::vector<long> Covisibility::UpdateLocalPoints(const std::vector<KeyFrameView*>& localKeyFrames) {
  Impl& m = *impl_;
  std::vector<int> kfs(localKeyFrames.size() + 1);
  size_t cap = 1;
  for (size_t i = 0; i < localKeyFrames.size(); ++i) { kfs[i] = m.pos(localKeyFrames[i], "Covisibility::UpdateLocalPoints"); cap += localKeyFrames[i]->mvKeys.size(); }
  const int off[2] = {0, (int)localKeyFrames.size()};
  std::vector<int> ids(cap);
  int n = 0;
  if (m.engine == HOST_CORE) {
    if (m.host.index.local_points(1, off, kfs.data(), (int)cap, ids.data(), &n)) throw std::runtime_error("Covisibility::UpdateLocalPoints: a key frame listed twice");
  } else {
    cms_ctx* c = m.ctx();
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (cms_covis_local_points(m.cv, c, 1, off, kfs.data(), (int)cap, ids.data(), &n) != CMS_OK) Impl::fail("cms_covis_local_points");
  }
  return std::vector<long>(ids.begin(), ids.begin() + n);
}

// ---- MapPointStore (src/MapPoint.cpp:243-308, :332-373)
struct MapPointStore::Impl {
  Engine engine;
  int max_keyframes, max_features, max_points;
  CmsMpHostStore* host = nullptr;            // HOST_CORE, made by the first Build (it wants the level scale factors)
  cms_kfstore* store = nullptr;              // DEVICE, made by the first Build
  cms_covis* cv = nullptr;
  cms_mpstore* mp = nullptr;
  std::vector<KeyFrameView*> members;
  std::map<KeyFrameView*, int> pos_of;
  Impl(Engine e, int K, int Fq, int P) : engine(e), max_keyframes(K), max_features(Fq), max_points(P) {}
  static cms_orb_params orb() {
    if (g_ctx_orb.nfeatures > 0) return g_ctx_orb;
    cms_orb_params o{};
    o.nfeatures = 2000; o.scale_factor = 1.2f; o.nlevels = 8; o.ini_th_fast = 20; o.min_th_fast = 7;
    return o;
  }
  static void fail(const char* who) { throw std::runtime_error(std::string(who) + " failed: " + cms_last_error()); }
  std::vector<int> ids32(const std::vector<long>& ids, const char* who) const {
    std::vector<int> out(ids.size() + 1);
    for (size_t i = 0; i < ids.size(); ++i) {
      if (ids[i] < 0 || ids[i] >= max_points) throw std::runtime_error(std::string(who) + ": an id outside the table");
      out[i] = (int)ids[i];
    }
    return out;
  }
};
MapPointStore::MapPointStore(Engine engine, int max_keyframes, int max_features, int max_points) : impl_(new Impl(engine, max_keyframes, max_features, max_points)) {}
MapPointStore::~MapPointStore() {
  if (impl_->mp) cms_mpstore_destroy(impl_->mp);
  if (impl_->cv) cms_covis_destroy(impl_->cv);
  if (impl_->store) cms_kfstore_destroy(impl_->store);
  delete impl_->host;
  delete impl_;
}
void MapPointStore::Build(const std::vector<KeyFrameView*>& members) {
  Impl& m = *impl_;
  if ((int)members.size() > m.max_keyframes) throw std::runtime_error("MapPointStore::Build: more key frames than max_keyframes");
  std::map<KeyFrameView*, int> pos_of;
  std::vector<int> slots(members.size() + 1);
  std::vector<std::vector<int>> rows(members.size());
  for (size_t i = 0; i < members.size(); ++i) {
    if (!members[i] || pos_of.count(members[i])) throw std::runtime_error("MapPointStore::Build: a null key frame, or one listed twice");
    const KeyFrameView& k = *members[i];
    if ((int)k.mvKeys.size() > m.max_features) throw std::runtime_error("MapPointStore::Build: a key frame with more features than max_features");
    pos_of[members[i]] = (int)i; slots[i] = (int)i;
    rows[i].resize(k.mvKeys.size() + 1);
    for (size_t f = 0; f < k.mvKeys.size(); ++f) {
      const bool bad = !k.mvbMapPointBad.empty() && k.mvbMapPointBad[f];
      rows[i][f] = (k.mvpMapPoints[f] >= 0 && k.mvpMapPoints[f] < m.max_points && !bad) ? (int)k.mvpMapPoints[f] : -1;
    }
  }
  const cms_orb_params orb = Impl::orb();
  if (m.engine == HOST_CORE) {
    if (!m.host) {
      float sf[16];      // ORBextractor's mvScaleFactor as cms_ctx_create forms it
      sf[0] = 1.0f;
      for (int l = 1; l < 16; ++l) sf[l] = (float)(sf[l - 1] * (double)orb.scale_factor);
      m.host = new CmsMpHostStore(m.max_keyframes, m.max_features, m.max_keyframes, m.max_points, orb.nlevels, sf);
    }
    for (size_t i = 0; i < members.size(); ++i) {
      const KeyFrameView& k = *members[i];
      std::vector<int> oct(k.mvKeys.size() + 1);
      std::vector<uint8_t> desc(32 * k.mvKeys.size() + 32);
      for (size_t f = 0; f < k.mvKeys.size(); ++f) { oct[f] = k.mvKeys[f].octave; std::memcpy(&desc[32 * f], k.mDescriptors.ptr<uint8_t>((int)f), 32); }
      float R[9], t[3], Ow[3];
      pose15_from_Tcw(k.Tcw, R, t, Ow);
      if (m.host->put((int)i, (int)k.mvKeys.size(), rows[i].data(), oct.data(), desc.data(), Ow)) throw std::runtime_error("MapPointStore::Build: bad key frame");
      std::memcpy(&m.host->Rcw[9 * i], R, 36); std::memcpy(&m.host->tcw[3 * i], t, 12);      // (the scene median depth reads the whole pose)
    }
    if (m.host->build((int)members.size(), slots.data())) throw std::runtime_error("MapPointStore::Build: a key frame names a map point twice");
  } else {
    cms_ctx* c = SharedContext(orb.nfeatures, orb.scale_factor, orb.nlevels, orb.ini_th_fast, orb.min_th_fast);
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!m.store && cms_kfstore_create(&m.store, c, m.max_keyframes, m.max_features, m.max_features) != CMS_OK) Impl::fail("cms_kfstore_create");
    if (!m.cv && cms_covis_create(&m.cv, m.store, m.max_keyframes) != CMS_OK) Impl::fail("cms_covis_create");
    if (!m.mp && cms_mpstore_create(&m.mp, m.store, m.max_points) != CMS_OK) Impl::fail("cms_mpstore_create");
    for (size_t i = 0; i < members.size(); ++i) {
      KfPack pack;
      cms_keyframe k = pack_keyframe(*members[i], pack);
      k.mp = rows[i].data();
      if (cms_kfstore_put(m.store, (int)i, &k) != CMS_OK) Impl::fail("cms_kfstore_put");
    }
    if (cms_covis_build(m.cv, (int)members.size(), slots.data()) != CMS_OK) Impl::fail("cms_covis_build");
  }
  m.members = members; m.pos_of.swap(pos_of);
}
void MapPointStore::SetMapPoints(const std::vector<MapPointView>& points) {
  Impl& m = *impl_;
  if (points.empty()) return;
  std::vector<long> ids(points.size());
  std::vector<float> pos(3 * points.size());
  std::vector<int> ref(points.size());
  for (size_t i = 0; i < points.size(); ++i) {
    ids[i] = points[i].id;
    std::memcpy(&pos[3 * i], points[i].pos, 12);
    auto it = m.pos_of.find(points[i].pRefKF);
    if (it == m.pos_of.end()) throw std::runtime_error("MapPointStore::SetMapPoints: pRefKF is not a member of the last Build");
    ref[i] = it->second;
  }
  const std::vector<int> id32 = m.ids32(ids, "MapPointStore::SetMapPoints");
  if (m.engine == HOST_CORE) {
    if (!m.host || m.host->set((int)points.size(), id32.data(), pos.data(), ref.data())) throw std::runtime_error("MapPointStore::SetMapPoints: an id twice (or no Build yet)");
  } else {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!m.mp || cms_mpstore_set(m.mp, (int)points.size(), id32.data(), pos.data(), ref.data()) != CMS_OK) Impl::fail("cms_mpstore_set");
  }
}
void MapPointStore::EraseMapPoints(const std::vector<long>& ids) {
  Impl& m = *impl_;
  if (ids.empty()) return;
  const std::vector<int> id32 = m.ids32(ids, "MapPointStore::EraseMapPoints");
  if (m.engine == HOST_CORE) {
    if (!m.host || m.host->erase((int)ids.size(), id32.data())) throw std::runtime_error("MapPointStore::EraseMapPoints: an id twice (or no Build yet)");
  } else {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!m.mp || cms_mpstore_erase(m.mp, (int)ids.size(), id32.data()) != CMS_OK) Impl::fail("cms_mpstore_erase");
  }
}
std::vector<unsigned char> MapPointStore::Refresh(const std::vector<long>& ids, int what) {
  Impl& m = *impl_;
  std::vector<unsigned char> status(ids.size() + 1);
  if (!ids.empty()) {
    const std::vector<int> id32 = m.ids32(ids, "MapPointStore::Refresh");
    if (m.engine == HOST_CORE) {
      if (!m.host || m.host->refresh((int)ids.size(), id32.data(), what, status.data())) throw std::runtime_error("MapPointStore::Refresh: an id twice, or a point that was never set");
    } else {
      std::lock_guard<std::mutex> lock(g_ctx_mutex);
      if (!m.mp || cms_mpstore_refresh(m.mp, m.cv, (int)ids.size(), id32.data(), what, status.data()) != CMS_OK) Impl::fail("cms_mpstore_refresh");
    }
  }
  status.resize(ids.size());
  return status;
}
std::vector<MapPointStore::Row> MapPointStore::Fetch(const std::vector<long>& ids) {
  Impl& m = *impl_;
  const size_t n = ids.size();
  std::vector<Row> out(n);
  if (n == 0) return out;
  const std::vector<int> id32 = m.ids32(ids, "MapPointStore::Fetch");
  std::vector<float> pos(3 * n), nrm(3 * n), mn(n), mx(n);
  std::vector<uint8_t> desc(32 * n);
  std::vector<int> bm(n), bf(n);
  if (m.engine == HOST_CORE) {
    if (!m.host || m.host->fetch((int)n, id32.data(), pos.data(), nrm.data(), mn.data(), mx.data(), desc.data(), bm.data(), bf.data())) throw std::runtime_error("MapPointStore::Fetch: no Build yet");
  } else {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!m.mp || cms_mpstore_fetch(m.mp, (int)n, id32.data(), pos.data(), nrm.data(), mn.data(), mx.data(), desc.data(), bm.data(), bf.data()) != CMS_OK) Impl::fail("cms_mpstore_fetch");
  }
  for (size_t i = 0; i < n; ++i) {
    Row& r = out[i];
    std::memcpy(r.pos, &pos[3 * i], 12); std::memcpy(r.normal, &nrm[3 * i], 12); std::memcpy(r.descriptor, &desc[32 * i], 32);
    r.minDistance = mn[i]; r.maxDistance = mx[i];
    r.pBestKF = (bm[i] >= 0 && (size_t)bm[i] < m.members.size()) ? m.members[(size_t)bm[i]] : nullptr;
    r.bestIdx = bf[i];
  }
  return out;
}

// ---- the local BA window from the resident stores (src/Optimizer.cpp:194-357; csrc/cms_ba_window_core.h)
MapPointStore::BAWindow MapPointStore::LocalBAWindow(const std::vector<KeyFrameView*>& lLocalKeyFrames) {
  Impl& m = *impl_;
  const size_t M = m.members.size();
  std::vector<int> local(lLocalKeyFrames.size() + 1);
  size_t cap_points = 1;
  for (size_t i = 0; i < lLocalKeyFrames.size(); ++i) {
    auto it = m.pos_of.find(lLocalKeyFrames[i]);
    if (it == m.pos_of.end()) throw std::runtime_error("MapPointStore::LocalBAWindow: a key frame is not a member of the last Build");
    local[i] = it->second;
    cap_points += lLocalKeyFrames[i]->mvKeys.size();
  }
  int first = -1;
  for (size_t i = 0; i < M; ++i) if (m.members[i]->mnId == 0) first = (int)i;
  const int cap_kf = (int)std::max(M, (size_t)1);
  size_t cap_edges = 8 * cap_points;
  CmsBaWindowCounts n = {0, 0, 0, 0};
  std::vector<int> kf_member((size_t)cap_kf), point_id(cap_points);
  BAWindow w;
  for (int attempt = 0; attempt < 2; ++attempt) {      // (the edges' number is not known before the first call: a second one with the counted size)
    w.poses.assign(7 * (size_t)cap_kf, 0.0); w.fixed.assign((size_t)cap_kf, 0); w.points.assign(3 * cap_points, 0.0);
    w.e_pose.assign(cap_edges, 0); w.e_point.assign(cap_edges, 0); w.e_obs.assign(2 * cap_edges, 0.0); w.e_invsig2.assign(cap_edges, 0.0); w.e_face.assign(cap_edges, 0);
    w.e_feat.assign(cap_edges, 0);
    int rc;
    if (m.engine == HOST_CORE) {
      if (!m.host) throw std::runtime_error("MapPointStore::LocalBAWindow: no Build yet");
      const cms_orb_params orb = Impl::orb();
      const CamModelGeneral* cam = CamModelGeneral::GetCamera();
      CmsBaWindowHostData D;
      D.F = cam->GetCubeFaceWidth(); D.cos_fov = cam->GetCosFovTh();
      float sc = 1.0f;      // mvInvLevelSigma2 as cms_ctx_create forms it
      for (int l = 0; l < 16; ++l) {
        if (l > 0) sc = (float)(sc * (double)orb.scale_factor);
        D.inv_sigma2[l] = l < orb.nlevels ? 1.0f / (l == 0 ? 1.0f : sc * sc) : 0.0f;
      }
      D.kx.resize(M); D.ky.resize(M); D.ray_z.resize(M); D.Rcw.resize(9 * M); D.tcw.resize(3 * M);
      for (size_t i = 0; i < M; ++i) {
        const KeyFrameView& k = *m.members[i];
        for (size_t f = 0; f < k.mvKeys.size(); ++f) { D.kx[i].push_back(k.mvKeys[f].pt.x); D.ky[i].push_back(k.mvKeys[f].pt.y); D.ray_z[i].push_back(k.mvKeyRays[f](2)); }
        float Ow[3];
        pose15_from_Tcw(k.Tcw, &D.Rcw[9 * i], &D.tcw[3 * i], Ow);
      }
      D.has_pos.resize(m.host->rows.size()); D.pos.resize(3 * m.host->rows.size());
      for (size_t i = 0; i < m.host->rows.size(); ++i) { D.has_pos[i] = m.host->rows[i].state & 1; std::memcpy(&D.pos[3 * i], m.host->rows[i].pos, 12); }
      const CmsBaWindowHostJob job = {(int)lLocalKeyFrames.size(), local.data(), first};
      const CmsBaWindowHostOut o = {cap_kf, (int)cap_points, (int)cap_edges, &n, kf_member.data(), point_id.data(), w.poses.data(), w.fixed.data(), w.points.data(),
                                    w.e_pose.data(), w.e_point.data(), w.e_obs.data(), w.e_invsig2.data(), w.e_face.data(), w.e_feat.data()};
      std::string why;
      rc = cms_ba_window_host(m.host->cv.index, D, 1, &job, o, &why);
      if (rc == -1) throw std::runtime_error("MapPointStore::LocalBAWindow: " + why);
    } else {
      std::lock_guard<std::mutex> lock(g_ctx_mutex);
      if (!m.mp) throw std::runtime_error("MapPointStore::LocalBAWindow: no Build yet");
      const cms_ba_window_job job = {(int)lLocalKeyFrames.size(), local.data(), first};
      cms_ba_window_counts c = {0, 0, 0, 0};
      rc = cms_covis_local_ba_windows(m.cv, m.mp, 1, &job, cap_kf, (int)cap_points, (int)cap_edges, &c, kf_member.data(), point_id.data(), w.poses.data(), w.fixed.data(),
                                      w.points.data(), w.e_pose.data(), w.e_point.data(), w.e_obs.data(), w.e_invsig2.data(), w.e_face.data(), w.e_feat.data());
      if (rc != CMS_OK && rc != CMS_ERR_OVERFLOW) Impl::fail("cms_covis_local_ba_windows");
      n = CmsBaWindowCounts{c.K, c.n_local, c.P, c.E};
    }
    if (rc == 0) break;
    if (attempt == 1 || n.K > cap_kf || (size_t)n.P > cap_points) throw std::runtime_error("MapPointStore::LocalBAWindow: the window does not fit its own bounds");
    cap_edges = (size_t)n.E;
  }
  w.nLocal = n.n_local;
  w.poses.resize(7 * (size_t)n.K); w.fixed.resize((size_t)n.K); w.points.resize(3 * (size_t)n.P);
  w.e_pose.resize((size_t)n.E); w.e_point.resize((size_t)n.E); w.e_obs.resize(2 * (size_t)n.E); w.e_invsig2.resize((size_t)n.E); w.e_face.resize((size_t)n.E); w.e_feat.resize((size_t)n.E);
  for (int k = 0; k < n.K; ++k) w.keyframes.push_back(m.members[(size_t)kf_member[(size_t)k]]);
  w.point_id.assign(point_id.begin(), point_id.begin() + n.P);
  return w;
}

void MapPointStore::WriteBack(const BAWindow& w) {
  Impl& m = *impl_;
  std::vector<int> slots, ids, ref;
  std::vector<float> R, t, Ow, pos;
  for (size_t k = 0; k < w.keyframes.size(); ++k) {   // Converter::toCvMat(SE3Quat) -> float 4x4 (Converter.cpp:53-104)
    if (w.fixed[k]) continue;                          // the reference rewrites local key frames only (:432-438)
    const double* q = &w.poses[7 * k + 3];
    const double x = q[0], y = q[1], z = q[2], s = q[3];
    const double Rd[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s), 2 * (x * y + z * s), 1 - 2 * (x * x + z * z),
                          2 * (y * z - x * s), 2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)};
    cv::Mat& T = w.keyframes[k]->Tcw;
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T.at<float>(r, c) = (float)Rd[3 * r + c]; T.at<float>(r, 3) = (float)w.poses[7 * k + r]; }
    float Rf[9], tf[3], Of[3];
    pose15_from_Tcw(T, Rf, tf, Of);
    slots.push_back(m.pos_of.at(w.keyframes[k]));
    R.insert(R.end(), Rf, Rf + 9); t.insert(t.end(), tf, tf + 3); Ow.insert(Ow.end(), Of, Of + 3);
  }
  for (size_t p = 0; p < w.point_id.size(); ++p) {
    ids.push_back((int)w.point_id[p]);
    for (int c = 0; c < 3; ++c) pos.push_back((float)w.points[3 * p + c]);
  }
  if (m.engine == HOST_CORE) {
    if (!slots.empty() && m.host->update_poses((int)slots.size(), slots.data(), Ow.data())) throw std::runtime_error("MapPointStore::WriteBack: bad key frame");
    for (size_t i = 0; i < slots.size(); ++i) { std::memcpy(&m.host->Rcw[9 * (size_t)slots[i]], &R[9 * i], 36); std::memcpy(&m.host->tcw[3 * (size_t)slots[i]], &t[3 * i], 12); }
    if (!ids.empty() && m.host->set((int)ids.size(), ids.data(), pos.data(), nullptr)) throw std::runtime_error("MapPointStore::WriteBack: bad point");
  } else {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!slots.empty() && cms_kfstore_update_poses(m.store, (int)slots.size(), slots.data(), R.data(), t.data(), Ow.data()) != CMS_OK) Impl::fail("cms_kfstore_update_poses");
    if (!ids.empty() && cms_mpstore_set(m.mp, (int)ids.size(), ids.data(), pos.data(), nullptr) != CMS_OK) Impl::fail("cms_mpstore_set");
  }
}

// ---- the points' counters, MapPointCulling, TrackedMapPoints and ComputeSceneMedianDepth (csrc/cms_mpstats_core.h).  HOST_CORE goes through the
// host build's entries on the same table (host_capi.cpp)
extern "C" {
int hm_mpstats_set_stats(void* mp, int n, const int* ids, const int* first_kf, const int* visible, const int* found);
int hm_mpstats_fetch_stats(void* mp, int n, const int* ids, int* visible, int* found, int* first_kf);
int hm_mpstats_count(void* mp, int which, int njobs, const int* off, const int* ids, const uint8_t* flag, int count_if);
int hm_mpstats_culling(void* mp, int njobs, const int* off, const int* ids, const int* current_kf, int th_obs, int apply, uint8_t* verdict);
int hm_mpstats_tracked_map_points(void* mp, int njobs, const int* job_member, const int* min_obs, int* count);
int hm_mpstats_scene_median_depth(void* mp, int n, const int* slots, int q, int store, float* depth, int* n_depths);
}
void MapPointStore::SetStatistics(const std::vector<MapPointStats>& stats) {
  Impl& m = *impl_;
  // one call per combination of columns: a point names the counters it sets
  for (int mask = 1; mask < 8; ++mask) {
    std::vector<long> ids;
    std::vector<int> first, vis, found;
    for (const MapPointStats& s : stats) {
      const int has = (s.nFirstKFid >= -1 ? 1 : 0) | (s.nVisible >= 0 ? 2 : 0) | (s.nFound >= 0 ? 4 : 0);
      if (has != mask) continue;
      ids.push_back(s.id); first.push_back(s.nFirstKFid); vis.push_back(s.nVisible); found.push_back(s.nFound);
    }
    if (ids.empty()) continue;
    const std::vector<int> id32 = m.ids32(ids, "MapPointStore::SetStatistics");
    const int n = (int)ids.size();
    const int* pf = (mask & 1) ? first.data() : nullptr;
    const int* pv = (mask & 2) ? vis.data() : nullptr;
    const int* pn = (mask & 4) ? found.data() : nullptr;
    if (m.engine == HOST_CORE) {
      if (!m.host || hm_mpstats_set_stats(m.host, n, id32.data(), pf, pv, pn)) throw std::runtime_error("MapPointStore::SetStatistics: a point that was never set, an id twice or a counter out of range");
    } else {
      std::lock_guard<std::mutex> lock(g_ctx_mutex);
      if (!m.mp || cms_mpstore_set_stats(m.mp, n, id32.data(), pf, pv, pn) != CMS_OK) Impl::fail("cms_mpstore_set_stats");
    }
  }
}
std::vector<MapPointStore::MapPointStats> MapPointStore::FetchStatistics(const std::vector<long>& ids) {
  Impl& m = *impl_;
  const int n = (int)ids.size();
  std::vector<MapPointStats> out(ids.size());
  if (n == 0) return out;
  const std::vector<int> id32 = m.ids32(ids, "MapPointStore::FetchStatistics");
  std::vector<int> vis(ids.size()), found(ids.size()), first(ids.size());
  if (m.engine == HOST_CORE) {
    if (!m.host || hm_mpstats_fetch_stats(m.host, n, id32.data(), vis.data(), found.data(), first.data())) throw std::runtime_error("MapPointStore::FetchStatistics: no Build yet");
  } else {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!m.mp || cms_mpstore_fetch_stats(m.mp, n, id32.data(), vis.data(), found.data(), first.data()) != CMS_OK) Impl::fail("cms_mpstore_fetch_stats");
  }
  for (size_t i = 0; i < ids.size(); ++i) out[i] = MapPointStats{ids[i], first[i], vis[i], found[i]};
  return out;
}
void MapPointStore::UpdateTrackStatistics(const std::vector<long>& localIds, const std::vector<unsigned char>& inView, const std::vector<long>& frameIds,
                                          const std::vector<unsigned char>& outlier) {
  Impl& m = *impl_;
  if (localIds.size() != inView.size() || frameIds.size() != outlier.size()) throw std::runtime_error("MapPointStore::UpdateTrackStatistics: a flag per id");
  struct Pass { const std::vector<long>* ids; const std::vector<unsigned char>* flag; int which, count_if; };
  const Pass passes[2] = {{&localIds, &inView, CMS_MP_VISIBLE, 1}, {&frameIds, &outlier, CMS_MP_FOUND, 0}};
  for (const Pass& p : passes) {
    if (p.ids->empty()) continue;
    std::vector<int> id32(p.ids->size());
    for (size_t i = 0; i < p.ids->size(); ++i) {
      const long id = (*p.ids)[i];
      if (id < -1 || id >= m.max_points) throw std::runtime_error("MapPointStore::UpdateTrackStatistics: an id outside the table");
      id32[i] = (int)id;
    }
    const int off[2] = {0, (int)id32.size()};
    if (m.engine == HOST_CORE) {
      if (!m.host || hm_mpstats_count(m.host, p.which, 1, off, id32.data(), p.flag->data(), p.count_if)) throw std::runtime_error("MapPointStore::UpdateTrackStatistics: a counted point that was never set");
    } else {
      const cms_orb_params orb = Impl::orb();
      cms_ctx* c = SharedContext(orb.nfeatures, orb.scale_factor, orb.nlevels, orb.ini_th_fast, orb.min_th_fast);
      std::lock_guard<std::mutex> lock(g_ctx_mutex);
      if (!m.mp || cms_mpstore_count(m.mp, c, p.which, 1, off, id32.data(), p.flag->data(), p.count_if) != CMS_OK) Impl::fail("cms_mpstore_count");
    }
  }
}
std::vector<unsigned char> MapPointStore::MapPointCulling(std::list<long>& recentIds, int currentKFid, int thObs) {
  Impl& m = *impl_;
  const std::vector<long> ids(recentIds.begin(), recentIds.end());
  std::vector<unsigned char> verdict(ids.size() + 1);
  if (!ids.empty()) {
    const std::vector<int> id32 = m.ids32(ids, "MapPointStore::MapPointCulling");
    const int off[2] = {0, (int)ids.size()};
    if (m.engine == HOST_CORE) {
      if (!m.host || hm_mpstats_culling(m.host, 1, off, id32.data(), &currentKFid, thObs, 1, verdict.data())) throw std::runtime_error("MapPointStore::MapPointCulling: an id twice (or no Build yet)");
    } else {
      std::lock_guard<std::mutex> lock(g_ctx_mutex);
      if (!m.mp || cms_mpstore_culling(m.mp, m.cv, 1, off, id32.data(), &currentKFid, thObs, 1, verdict.data()) != CMS_OK) Impl::fail("cms_mpstore_culling");
    }
  }
  verdict.resize(ids.size());
  // SetBadFlag on the views (MapPoint.cpp:115-136), then the list (LocalMapping.cpp:184-205): only a point of verdict 0 stays
  std::set<long> bad;
  size_t i = 0;
  for (auto it = recentIds.begin(); it != recentIds.end(); ++i) {
    if (verdict[i] == CMS_MP_BAD_RATIO || verdict[i] == CMS_MP_BAD_FEW_OBS) bad.insert(*it);
    if (verdict[i] != CMS_MP_STAYS) it = recentIds.erase(it); else ++it;
  }
  if (!bad.empty())
    for (KeyFrameView* k : m.members)
      for (long& id : k->mvpMapPoints) if (id >= 0 && bad.count(id)) id = -1;
  return verdict;
}
int MapPointStore::TrackedMapPoints(KeyFrameView* pKF, int minObs) {
  Impl& m = *impl_;
  auto it = m.pos_of.find(pKF);
  if (it == m.pos_of.end()) throw std::runtime_error("MapPointStore::TrackedMapPoints: not a key frame of the last Build");
  const int member = it->second;
  int count = 0;
  if (m.engine == HOST_CORE) {
    if (!m.host || hm_mpstats_tracked_map_points(m.host, 1, &member, &minObs, &count)) throw std::runtime_error("MapPointStore::TrackedMapPoints: no Build yet");
  } else {
    const cms_orb_params orb = Impl::orb();
    cms_ctx* c = SharedContext(orb.nfeatures, orb.scale_factor, orb.nlevels, orb.ini_th_fast, orb.min_th_fast);
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!m.cv || cms_covis_tracked_map_points(m.cv, c, 1, &member, &minObs, &count) != CMS_OK) Impl::fail("cms_covis_tracked_map_points");
  }
  return count;
}
float MapPointStore::ComputeSceneMedianDepth(KeyFrameView* pKF, int q) {
  Impl& m = *impl_;
  auto it = m.pos_of.find(pKF);
  if (it == m.pos_of.end()) throw std::runtime_error("MapPointStore::ComputeSceneMedianDepth: not a key frame of the last Build");
  const int slot = it->second;      // (Build puts member i into slot i)
  float depth = -1.0f;
  int n = 0;
  if (m.engine == HOST_CORE) {
    if (!m.host || hm_mpstats_scene_median_depth(m.host, 1, &slot, q, 0, &depth, &n)) throw std::runtime_error("MapPointStore::ComputeSceneMedianDepth: q < 1 (or no Build yet)");
  } else {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!m.mp || cms_kfstore_scene_median_depth(m.store, m.mp, 1, &slot, q, 0, &depth, &n) != CMS_OK) Impl::fail("cms_kfstore_scene_median_depth");
  }
  return depth;
}

void Optimizer::LocalBundleAdjustment(MapPointStore& mps, MapPointStore::BAWindow* win, bool* pbStopFlag) {
  const int K = (int)win->keyframes.size(), P = (int)win->point_id.size(), E = (int)win->e_pose.size();
  win->toErase.clear();
  if (K == 0 || P == 0 || E == 0) return;
  if (pbStopFlag && *pbStopFlag) return;                                       // :359-361
  std::vector<uint8_t> flags((size_t)E);
  const double f = CamModelGeneral::GetCamera()->Get_fx();
  const int rc = cms_ba_run(0, K, win->poses.data(), win->fixed.data(), P, win->points.data(), E, win->e_pose.data(), win->e_point.data(), win->e_obs.data(),
                            win->e_invsig2.data(), win->e_face.data(), f, f, f, f, 5, 10, reinterpret_cast<const volatile uint8_t*>(pbStopFlag), flags.data(), nullptr);
  if (rc < 0) throw std::runtime_error(std::string("cms_ba_run: ") + cms_last_error());
  if (rc == 1) return;
  for (int e = 0; e < E; ++e) if (flags[(size_t)e]) win->toErase.push_back(std::make_pair(win->keyframes[(size_t)win->e_pose[(size_t)e]], win->e_feat[(size_t)e]));  // :399-412
  mps.WriteBack(*win);
}

}  // namespace CubemapSLAM
