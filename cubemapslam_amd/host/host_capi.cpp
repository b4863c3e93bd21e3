// host_capi.cpp -- flat C entry points around the C++ mirror classes (cubemap_hot_path.h) so the Python test-suite can
// drive them exactly the way a C++ caller (Tracking / LocalMapping) would.  Test plumbing, not part of the boundary.
#include <cstring>
#include <memory>
#include <stdexcept>
#include "cubemap_hot_path.h"
#include "io_formats.h"
#include "../csrc/cms_vocab_core.h"
#include "../csrc/cms_kfdb_core.h"
#include "../csrc/cms_covis_core.h"
#include "../csrc/cms_mappoint_core.h"
#include "../csrc/cms_mpstats_core.h"
#include "../csrc/cms_ba_window_core.h"
using namespace CubemapSLAM;

static thread_local std::string g_err;
extern "C" const char* hm_last_error() { return g_err.c_str(); }
#define HM_TRY(...) try { __VA_ARGS__ } catch (const std::exception& e) { g_err = e.what(); return -1; }

extern "C" int hm_set_camera(const cms_camera* c) {
  HM_TRY(
    const double cde[5] = {c->c, c->d, c->e, c->u0, c->v0};
    std::vector<double> pol(c->pol, c->pol + 5), inv(c->invpol, c->invpol + 12);
    const double h = c->face / 2.0;
    CamModelGeneral::GetCamera()->SetCamParams(cde, pol, inv, c->Iw, c->Ih, h, h, h, h, c->face, c->face, c->fov_deg);
    return 0;)
}
extern "C" int hm_remap(const uint8_t* fish, int fstride, uint8_t* cube, int cstride) {
  HM_TRY(
    CamModelGeneral* cam = CamModelGeneral::GetCamera();
    System sys;
    sys.CreateUndistortRectifyMap();
    cv::Mat f(cam->GetFisheyeHeight(), cam->GetFisheyeWidth(), cv::CV_8U, (void*)fish, (size_t)fstride);
    const int W = 3 * cam->GetCubeFaceWidth();
    cv::Mat c(W, W, cv::CV_8U, cube, (size_t)cstride);
    sys.CvtFisheyeToCubeMap_reverseQuery_withInterpolation(c, f, cv::INTER_LINEAR);
    return 0;)
}
extern "C" int hm_extract(int nfeatures, float scale, int nlevels, int ini_th, int min_th, const uint8_t* img, int stride,
                          const uint8_t* mask, int mstride, cms_keypoint* kps, uint8_t* desc, int cap) {
  HM_TRY(
    const int W = 3 * CamModelGeneral::GetCamera()->GetCubeFaceWidth();
    ORBextractor ex(nfeatures, scale, nlevels, ini_th, min_th);
    cv::Mat image(W, W, cv::CV_8U, (void*)img, (size_t)stride), m(W, W, cv::CV_8U, (void*)mask, (size_t)mstride), d;
    std::vector<cv::KeyPoint> keys;
    ex(image, m, keys, d);
    const int n = (int)keys.size();
    for (int i = 0; i < n && i < cap; ++i) {
      kps[i] = cms_keypoint{keys[i].pt.x, keys[i].pt.y, keys[i].size, keys[i].angle, keys[i].response, keys[i].octave};
      std::memcpy(desc + (size_t)i * 32, d.ptr<uint8_t>(i), 32);
    }
    return n;)
}
// ORBextractor::mvImagePyramid (ORBExtractor.h:89): extract with mbKeepImagePyramid and hand level `level` back (w x h written to wh)
extern "C" int hm_extract_pyramid_level(int nfeatures, float scale, int nlevels, int ini_th, int min_th, const uint8_t* img, int stride, const uint8_t* mask,
                                        int mstride, int level, uint8_t* out, int out_stride, int* wh) {
  HM_TRY(
    const int W = 3 * CamModelGeneral::GetCamera()->GetCubeFaceWidth();
    ORBextractor ex(nfeatures, scale, nlevels, ini_th, min_th);
    ex.mbKeepImagePyramid = true;
    cv::Mat image(W, W, cv::CV_8U, (void*)img, (size_t)stride), m(W, W, cv::CV_8U, (void*)mask, (size_t)mstride), d;
    std::vector<cv::KeyPoint> keys;
    ex(image, m, keys, d);
    if (level < 0 || level >= (int)ex.mvImagePyramid.size()) return -1;
    const cv::Mat& lv = ex.mvImagePyramid[level];
    wh[0] = lv.cols; wh[1] = lv.rows;
    for (int r = 0; r < lv.rows; ++r) std::memcpy(out + (size_t)r * out_stride, lv.ptr<uint8_t>(r), (size_t)lv.cols);
    return (int)keys.size();)
}
// frame-to-frame SearchByProjection: returns matches; cur_mp[j] receives the matched map-point id or -1
extern "C" int hm_search_by_projection(int ncur, const cms_keypoint* cur_k, const uint8_t* cur_d, long* cur_mp, int nlast,
                                       const cms_keypoint* last_k, const uint8_t* last_d, const long* last_mp, const float* proj_xy,
                                       const float* scale_factors, int nlevels, float th, float nnratio, int check_ori) {
  HM_TRY(
    FrameView cur, last;
    auto fill = [](FrameView& f, int n, const cms_keypoint* k, const uint8_t* d) {
      f.mvKeys.resize(n);
      f.mDescriptors.create(n > 0 ? n : 1, 32, cv::CV_8U);
      for (int i = 0; i < n; ++i) {
        f.mvKeys[i].pt = cv::Point2f(k[i].x, k[i].y); f.mvKeys[i].angle = k[i].angle; f.mvKeys[i].octave = k[i].octave;
        std::memcpy(f.mDescriptors.ptr<uint8_t>(i), d + (size_t)i * 32, 32);
      }
    };
    fill(cur, ncur, cur_k, cur_d); fill(last, nlast, last_k, last_d);
    cur.mvpMapPoints.assign(cur_mp, cur_mp + ncur);
    last.mvpMapPoints.assign(last_mp, last_mp + nlast);
    last.mvbOutlier.assign(nlast, 0);
    last.projInCurrent.resize(nlast);
    for (int i = 0; i < nlast; ++i) last.projInCurrent[i] = cv::Point2f(proj_xy[2 * i], proj_xy[2 * i + 1]);
    cur.mvScaleFactors.assign(scale_factors, scale_factors + nlevels);
    ORBMatcher matcher(nnratio, check_ori != 0);
    const int n = matcher.SearchByProjection(cur, last, th, true);
    for (int j = 0; j < ncur; ++j) cur_mp[j] = cur.mvpMapPoints[j];
    return n;)
}
// frame-to-frame SearchByProjection, device path: the last frame's map points come with position + descriptor, the current frame with its pose
extern "C" int hm_search_by_projection_pose(int ncur, const cms_keypoint* cur_k, const uint8_t* cur_d, long* cur_mp, float* Tcw, int nlast,
                                            const cms_keypoint* last_k, const long* last_mp, const uint8_t* last_outlier, const float* mp_pos,
                                            const uint8_t* mp_desc, float th, int check_ori) {
  HM_TRY(
    FrameView cur, last;
    cur.mvKeys.resize(ncur); cur.mDescriptors.create(ncur > 0 ? ncur : 1, 32, cv::CV_8U);
    for (int i = 0; i < ncur; ++i) {
      cur.mvKeys[i].pt = cv::Point2f(cur_k[i].x, cur_k[i].y); cur.mvKeys[i].angle = cur_k[i].angle; cur.mvKeys[i].octave = cur_k[i].octave;
      std::memcpy(cur.mDescriptors.ptr<uint8_t>(i), cur_d + (size_t)i * 32, 32);
    }
    cur.mvpMapPoints.assign(cur_mp, cur_mp + ncur);
    cur.mTcw = cv::Mat(4, 4, cv::CV_32F, Tcw, 16);
    last.mvKeys.resize(nlast); last.mvMapPointPos.resize(nlast); last.mMapPointDescriptors.create(nlast > 0 ? nlast : 1, 32, cv::CV_8U);
    for (int i = 0; i < nlast; ++i) {
      last.mvKeys[i].pt = cv::Point2f(last_k[i].x, last_k[i].y); last.mvKeys[i].angle = last_k[i].angle; last.mvKeys[i].octave = last_k[i].octave;
      for (int c = 0; c < 3; ++c) last.mvMapPointPos[i].v[c] = mp_pos[3 * (size_t)i + c];
      std::memcpy(last.mMapPointDescriptors.ptr<uint8_t>(i), mp_desc + (size_t)i * 32, 32);
    }
    last.mvpMapPoints.assign(last_mp, last_mp + nlast);
    last.mvbOutlier.assign(last_outlier, last_outlier + nlast);
    ORBMatcher matcher(0.9f, check_ori != 0);
    const int n = matcher.SearchByProjection(cur, last, th, true);
    for (int j = 0; j < ncur; ++j) cur_mp[j] = cur.mvpMapPoints[j];
    return n;)
}
// Tracking::SearchLocalPoints: Tcw 16 floats (row major 4x4); map points as flat arrays; outputs per map point + cur_mp[j] updated
extern "C" int hm_search_local_points(int ncur, const cms_keypoint* cur_k, const uint8_t* cur_d, long* cur_mp, const float* scale_factors, int nlevels,
                                      float* Tcw, int nmp, const long* mp_id, const float* pos, const float* normal, const float* min_dist,
                                      const float* max_dist, const uint8_t* mp_desc, float th, float nnratio, uint8_t* in_view, float* proj_xy,
                                      int* level, float* view_cos) {
  HM_TRY(
    FrameView cur;
    cur.mvKeys.resize(ncur);
    cur.mDescriptors.create(ncur > 0 ? ncur : 1, 32, cv::CV_8U);
    for (int i = 0; i < ncur; ++i) {
      cur.mvKeys[i].pt = cv::Point2f(cur_k[i].x, cur_k[i].y); cur.mvKeys[i].angle = cur_k[i].angle; cur.mvKeys[i].octave = cur_k[i].octave;
      std::memcpy(cur.mDescriptors.ptr<uint8_t>(i), cur_d + (size_t)i * 32, 32);
    }
    cur.mvpMapPoints.assign(cur_mp, cur_mp + ncur);
    cur.mvScaleFactors.assign(scale_factors, scale_factors + nlevels);
    cur.mTcw = cv::Mat(4, 4, cv::CV_32F, Tcw, 16);
    std::vector<MapPointView> mps(nmp);
    for (int i = 0; i < nmp; ++i) {
      mps[i].mnId = mp_id[i];
      mps[i].mWorldPos = cv::Mat(3, 1, cv::CV_32F, const_cast<float*>(pos) + 3 * (size_t)i, 4);
      mps[i].mNormalVector = cv::Mat(3, 1, cv::CV_32F, const_cast<float*>(normal) + 3 * (size_t)i, 4);
      mps[i].mfMinDistance = min_dist[i]; mps[i].mfMaxDistance = max_dist[i];
      mps[i].mDescriptor = cv::Mat(1, 32, cv::CV_8U, const_cast<uint8_t*>(mp_desc) + 32 * (size_t)i, 32);
    }
    const int n = Tracking::SearchLocalPoints(cur, mps, th, nnratio);
    for (int j = 0; j < ncur; ++j) cur_mp[j] = cur.mvpMapPoints[j];
    for (int i = 0; i < nmp; ++i) {
      in_view[i] = mps[i].mbTrackInView; proj_xy[2 * i] = mps[i].mTrackProjX; proj_xy[2 * i + 1] = mps[i].mTrackProjY;
      level[i] = mps[i].mnTrackScaleLevel; view_cos[i] = mps[i].mTrackViewCos;
    }
    return n;)
}
// ORBMatcher::SearchByProjection(F, vpMapPoints, th) through the mirror: the caller marks the points in view (what Frame::isInFrustum left in them)
extern "C" int hm_search_by_projection_map(int ncur, const cms_keypoint* cur_k, const uint8_t* cur_d, long* cur_mp, const float* scale_factors, int nlevels,
                                           float* Tcw, int nmp, const long* mp_id, const float* pos, const float* normal, const float* min_dist,
                                           const float* max_dist, const uint8_t* mp_desc, const uint8_t* in_view, float th, float nnratio) {
  HM_TRY(
    FrameView cur;
    cur.mvKeys.resize(ncur);
    cur.mDescriptors.create(ncur > 0 ? ncur : 1, 32, cv::CV_8U);
    for (int i = 0; i < ncur; ++i) {
      cur.mvKeys[i].pt = cv::Point2f(cur_k[i].x, cur_k[i].y); cur.mvKeys[i].angle = cur_k[i].angle; cur.mvKeys[i].octave = cur_k[i].octave;
      std::memcpy(cur.mDescriptors.ptr<uint8_t>(i), cur_d + (size_t)i * 32, 32);
    }
    cur.mvpMapPoints.assign(cur_mp, cur_mp + ncur);
    cur.mvScaleFactors.assign(scale_factors, scale_factors + nlevels);
    cur.mTcw = cv::Mat(4, 4, cv::CV_32F, Tcw, 16);
    std::vector<MapPointView> mps(nmp);
    for (int i = 0; i < nmp; ++i) {
      mps[i].mnId = mp_id[i];
      mps[i].mWorldPos = cv::Mat(3, 1, cv::CV_32F, const_cast<float*>(pos) + 3 * (size_t)i, 4);
      mps[i].mNormalVector = cv::Mat(3, 1, cv::CV_32F, const_cast<float*>(normal) + 3 * (size_t)i, 4);
      mps[i].mfMinDistance = min_dist[i]; mps[i].mfMaxDistance = max_dist[i];
      mps[i].mDescriptor = cv::Mat(1, 32, cv::CV_8U, const_cast<uint8_t*>(mp_desc) + 32 * (size_t)i, 32);
      mps[i].mbTrackInView = in_view[i] != 0;
    }
    ORBMatcher matcher(nnratio, true);
    const int n = matcher.SearchByProjection(cur, mps, th);
    for (int j = 0; j < ncur; ++j) cur_mp[j] = cur.mvpMapPoints[j];
    return n;)
}
// ORBMatcher::SearchForInitialization through the mirror; prev_xy (n1 x 2) is vbPrevMatched, in / out
extern "C" int hm_search_for_initialization(int n1, const cms_keypoint* k1, const uint8_t* d1, int n2, const cms_keypoint* k2, const uint8_t* d2,
                                            float* prev_xy, int window, float nnratio, int check_ori, int* matches12) {
  HM_TRY(
    FrameView f1, f2;
    auto fill = [](FrameView& f, int n, const cms_keypoint* k, const uint8_t* d) {
      f.mvKeys.resize(n);
      f.mDescriptors.create(n > 0 ? n : 1, 32, cv::CV_8U);
      for (int i = 0; i < n; ++i) {
        f.mvKeys[i].pt = cv::Point2f(k[i].x, k[i].y); f.mvKeys[i].angle = k[i].angle; f.mvKeys[i].octave = k[i].octave; f.mvKeys[i].size = k[i].size;
        f.mvKeys[i].response = k[i].response;
        std::memcpy(f.mDescriptors.ptr<uint8_t>(i), d + (size_t)i * 32, 32);
      }
    };
    fill(f1, n1, k1, d1); fill(f2, n2, k2, d2);
    std::vector<cv::Point2f> prev(n1);
    for (int i = 0; i < n1; ++i) prev[i] = cv::Point2f(prev_xy[2 * i], prev_xy[2 * i + 1]);
    std::vector<int> m12;
    ORBMatcher matcher(nnratio, check_ori != 0);
    const int n = matcher.SearchForInitialization(f1, f2, prev, m12, window);
    for (int i = 0; i < n1; ++i) { matches12[i] = m12[i]; prev_xy[2 * i] = prev[i].x; prev_xy[2 * i + 1] = prev[i].y; }
    return n;)
}
// ORBMatcher::SearchForTriangulation through the mirror: two key frames in hm_create_new_map_points' flat layout (nkf = 2), E12 row major
extern "C" int hm_search_for_triangulation(const int* feat_off, const cms_keypoint* kps, const uint8_t* desc, const float* rays, const long* mp,
                                           float* Tcw, const int* node_off2, const int* node_id, const int* node_cnt, const int* node_feat,
                                           float* E12, int check_ori, int cap, int* out_idx1, int* out_idx2) {
  HM_TRY(
    std::vector<KeyFrameView> kfs(2);
    size_t nf_cursor = 0;
    for (int k = 0; k < 2; ++k) {
      KeyFrameView& v = kfs[k];
      const int f0 = feat_off[k], n = feat_off[k + 1] - f0;
      v.mnId = k; v.mvKeys.resize(n); v.mvKeyRays.resize(n); v.mvpMapPoints.assign(mp + f0, mp + f0 + n);
      v.mDescriptors.create(n > 0 ? n : 1, 32, cv::CV_8U);
      for (int i = 0; i < n; ++i) {
        const cms_keypoint& s = kps[f0 + i];
        v.mvKeys[i].pt = cv::Point2f(s.x, s.y); v.mvKeys[i].angle = s.angle; v.mvKeys[i].octave = s.octave;
        std::memcpy(v.mDescriptors.ptr<uint8_t>(i), desc + 32 * (size_t)(f0 + i), 32);
        for (int c = 0; c < 3; ++c) v.mvKeyRays[i].v[c] = rays[3 * (size_t)(f0 + i) + c];
      }
      v.Tcw = cv::Mat(4, 4, cv::CV_32F, Tcw + 16 * (size_t)k, 16);
      for (int e = node_off2[k]; e < node_off2[k + 1]; ++e) {
        std::vector<unsigned> fl(node_feat + nf_cursor, node_feat + nf_cursor + node_cnt[e]);
        nf_cursor += (size_t)node_cnt[e];
        v.mFeatVec.emplace_back((unsigned)node_id[e], std::move(fl));
      }
    }
    std::vector<std::pair<size_t, size_t>> pairs;
    ORBMatcher matcher(0.6f, check_ori != 0);
    const int n = matcher.SearchForTriangulation(kfs[0], kfs[1], cv::Mat(3, 3, cv::CV_32F, E12, 12), pairs);
    for (int i = 0; i < (int)pairs.size() && i < cap; ++i) { out_idx1[i] = (int)pairs[i].first; out_idx2[i] = (int)pairs[i].second; }
    return n;)
}
// ORBMatcher::SearchByBoW(pKF, F, vpMapPointMatches) through the mirror: the key frame (nk features, map-point ids mp (-1 = none), bad flags or NULL,
// FeatureVector as CSR) and the frame (n features, FeatureVector as CSR); out_mp[n] = the matched map point's id or -1
extern "C" int hm_search_by_bow(int nk, const cms_keypoint* kk, const uint8_t* kd, const long* mp, const uint8_t* bad, int kn_nodes, const int* k_nid,
                                const int* k_noff, const int* k_nfeat, int n, const cms_keypoint* fk, const uint8_t* fd, int f_nodes, const int* f_nid,
                                const int* f_noff, const int* f_nfeat, float nnratio, int check_ori, long* out_mp) {
  HM_TRY(
    KeyFrameView kf;
    FrameView f;
    auto keys = [](std::vector<cv::KeyPoint>& v, cv::Mat& d, int m, const cms_keypoint* k, const uint8_t* desc) {
      v.resize(m);
      d.create(m > 0 ? m : 1, 32, cv::CV_8U);
      for (int i = 0; i < m; ++i) {
        v[i].pt = cv::Point2f(k[i].x, k[i].y); v[i].angle = k[i].angle; v[i].octave = k[i].octave; v[i].size = k[i].size; v[i].response = k[i].response;
        std::memcpy(d.ptr<uint8_t>(i), desc + (size_t)i * 32, 32);
      }
    };
    auto featvec = [](std::vector<std::pair<unsigned, std::vector<unsigned>>>& fv, int nn, const int* nid, const int* noff, const int* nfeat) {
      for (int e = 0; e < nn; ++e) fv.emplace_back((unsigned)nid[e], std::vector<unsigned>(nfeat + noff[e], nfeat + noff[e + 1]));
    };
    keys(kf.mvKeys, kf.mDescriptors, nk, kk, kd);
    kf.mvpMapPoints.assign(mp, mp + nk);
    if (bad) kf.mvbMapPointBad.assign(bad, bad + nk);
    featvec(kf.mFeatVec, kn_nodes, k_nid, k_noff, k_nfeat);
    keys(f.mvKeys, f.mDescriptors, n, fk, fd);
    featvec(f.mFeatVec, f_nodes, f_nid, f_noff, f_nfeat);
    std::vector<long> m;
    ORBMatcher matcher(nnratio, check_ori != 0);
    const int nm = matcher.SearchByBoW(kf, f, m);
    for (int i = 0; i < n; ++i) out_mp[i] = m[i];
    return nm;)
}
// ORBMatcher::SearchByBoW(pKF1, pKF2, vpMatches12) through the mirror: two key frames (n features, map-point ids mp (-1 = none), bad flags or NULL,
// FeatureVector as CSR); out_mp[n1] = the id of key frame 2's matched map point or -1
extern "C" int hm_search_by_bow_keyframes(int n1, const cms_keypoint* k1, const uint8_t* d1, const long* mp1, const uint8_t* bad1, int nodes1, const int* nid1,
                                          const int* noff1, const int* nfeat1, int n2, const cms_keypoint* k2, const uint8_t* d2, const long* mp2,
                                          const uint8_t* bad2, int nodes2, const int* nid2, const int* noff2, const int* nfeat2, float nnratio, int check_ori,
                                          long* out_mp) {
  HM_TRY(
    auto view = [](KeyFrameView& kf, int n, const cms_keypoint* k, const uint8_t* desc, const long* mp, const uint8_t* bad, int nn, const int* nid, const int* noff,
                   const int* nfeat) {
      kf.mvKeys.resize(n);
      kf.mDescriptors.create(n > 0 ? n : 1, 32, cv::CV_8U);
      for (int i = 0; i < n; ++i) {
        kf.mvKeys[i].pt = cv::Point2f(k[i].x, k[i].y); kf.mvKeys[i].angle = k[i].angle; kf.mvKeys[i].octave = k[i].octave; kf.mvKeys[i].size = k[i].size;
        kf.mvKeys[i].response = k[i].response;
        std::memcpy(kf.mDescriptors.ptr<uint8_t>(i), desc + (size_t)i * 32, 32);
      }
      kf.mvpMapPoints.assign(mp, mp + n);
      if (bad) kf.mvbMapPointBad.assign(bad, bad + n);
      for (int e = 0; e < nn; ++e) kf.mFeatVec.emplace_back((unsigned)nid[e], std::vector<unsigned>(nfeat + noff[e], nfeat + noff[e + 1]));
    };
    KeyFrameView kf1;
    KeyFrameView kf2;
    view(kf1, n1, k1, d1, mp1, bad1, nodes1, nid1, noff1, nfeat1);
    view(kf2, n2, k2, d2, mp2, bad2, nodes2, nid2, noff2, nfeat2);
    std::vector<long> m;
    ORBMatcher matcher(nnratio, check_ori != 0);
    const int nm = matcher.SearchByBoW(kf1, kf2, m);
    for (int i = 0; i < n1; ++i) out_mp[i] = m[i];
    return nm;)
}
// ORBMatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) through the mirror: the key frame (nk key points, map-point ids mp
// (-1 = none), bad flags or NULL, and per key point the map point's position / mfMinDistance / mfMaxDistance / descriptor), sAlreadyFound as nfound
// ids, the frame (n key points, frame_mp[n] = mvpMapPoints as ids, in/out) and its pose Tcw (16 floats, row major)
extern "C" int hm_search_by_projection_keyframe(int nk, const cms_keypoint* kk, const long* mp, const uint8_t* bad, const float* mp_pos, const float* mp_min,
                                                const float* mp_max, const uint8_t* mp_desc, int nfound, const long* found, int n, const cms_keypoint* fk,
                                                const uint8_t* fd, long* frame_mp, float* Tcw, float th, int orb_dist, int check_ori) {
  HM_TRY(
    KeyFrameView kf;
    FrameView f;
    kf.mvKeys.resize(nk); kf.mvMapPoints.resize(nk);
    kf.mvpMapPoints.assign(mp, mp + nk);
    if (bad) kf.mvbMapPointBad.assign(bad, bad + nk);
    for (int i = 0; i < nk; ++i) {
      kf.mvKeys[i].pt = cv::Point2f(kk[i].x, kk[i].y); kf.mvKeys[i].angle = kk[i].angle; kf.mvKeys[i].octave = kk[i].octave;
      MapPointView& v = kf.mvMapPoints[i];
      v.mnId = mp[i]; v.mfMinDistance = mp_min[i]; v.mfMaxDistance = mp_max[i];
      v.mWorldPos.create(3, 1, cv::CV_32F);
      for (int c = 0; c < 3; ++c) v.mWorldPos.at<float>(c, 0) = mp_pos[3 * (size_t)i + c];
      v.mDescriptor.create(1, 32, cv::CV_8U);
      std::memcpy(v.mDescriptor.ptr<uint8_t>(0), mp_desc + 32 * (size_t)i, 32);
    }
    f.mvKeys.resize(n);
    f.mDescriptors.create(n > 0 ? n : 1, 32, cv::CV_8U);
    for (int i = 0; i < n; ++i) {
      f.mvKeys[i].pt = cv::Point2f(fk[i].x, fk[i].y); f.mvKeys[i].angle = fk[i].angle; f.mvKeys[i].octave = fk[i].octave; f.mvKeys[i].size = fk[i].size;
      f.mvKeys[i].response = fk[i].response;
      std::memcpy(f.mDescriptors.ptr<uint8_t>(i), fd + (size_t)i * 32, 32);
    }
    f.mvpMapPoints.assign(frame_mp, frame_mp + n);
    f.mTcw = cv::Mat(4, 4, cv::CV_32F, Tcw, 16);
    const std::set<long> sFound(found, found + nfound);
    ORBMatcher matcher(0.9f, check_ori != 0);
    const int nm = matcher.SearchByProjection(f, kf, sFound, th, orb_dist);
    for (int i = 0; i < n; ++i) frame_mp[i] = f.mvpMapPoints[i];
    return nm;)
}
// ORBMatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) through the mirror: per key frame n key points with descriptors, its pose Tcw
// (16 floats, row major), map-point ids mp (-1 = none), bad flags or NULL, and per key point the map point's position / mfMinDistance /
// mfMaxDistance / descriptor; R12 9 floats row major, t12 3; matches12[n1] = vpMatches12 as ids, in/out
extern "C" int hm_search_by_sim3(int n1, const cms_keypoint* k1, const uint8_t* d1, float* Tcw1, const long* mp1, const uint8_t* bad1, const float* pos1, const float* min1,
                                 const float* max1, const uint8_t* mpd1, int n2, const cms_keypoint* k2, const uint8_t* d2, float* Tcw2, const long* mp2,
                                 const uint8_t* bad2, const float* pos2, const float* min2, const float* max2, const uint8_t* mpd2, float s12, float* R12, float* t12,
                                 float th, int z_as_written, long* matches12) {
  HM_TRY(
    auto view = [](KeyFrameView& kf, int n, const cms_keypoint* k, const uint8_t* desc, float* Tcw, const long* mp, const uint8_t* bad, const float* pos, const float* mn,
                   const float* mx, const uint8_t* mpd) {
      kf.mvKeys.resize(n); kf.mvMapPoints.resize(n);
      kf.mDescriptors.create(n > 0 ? n : 1, 32, cv::CV_8U);
      kf.mvpMapPoints.assign(mp, mp + n);
      if (bad) kf.mvbMapPointBad.assign(bad, bad + n);
      kf.Tcw = cv::Mat(4, 4, cv::CV_32F, Tcw, 16);
      for (int i = 0; i < n; ++i) {
        kf.mvKeys[i].pt = cv::Point2f(k[i].x, k[i].y); kf.mvKeys[i].angle = k[i].angle; kf.mvKeys[i].octave = k[i].octave; kf.mvKeys[i].size = k[i].size;
        kf.mvKeys[i].response = k[i].response;
        std::memcpy(kf.mDescriptors.ptr<uint8_t>(i), desc + (size_t)i * 32, 32);
        MapPointView& v = kf.mvMapPoints[i];
        v.mnId = mp[i]; v.mfMinDistance = mn[i]; v.mfMaxDistance = mx[i];
        v.mWorldPos.create(3, 1, cv::CV_32F);
        for (int c = 0; c < 3; ++c) v.mWorldPos.at<float>(c, 0) = pos[3 * (size_t)i + c];
        v.mDescriptor.create(1, 32, cv::CV_8U);
        std::memcpy(v.mDescriptor.ptr<uint8_t>(0), mpd + 32 * (size_t)i, 32);
      }
    };
    KeyFrameView kf1;
    KeyFrameView kf2;
    view(kf1, n1, k1, d1, Tcw1, mp1, bad1, pos1, min1, max1, mpd1);
    view(kf2, n2, k2, d2, Tcw2, mp2, bad2, pos2, min2, max2, mpd2);
    std::vector<long> m(matches12, matches12 + n1);
    ORBMatcher matcher(0.75f, true);
    const int nm = matcher.SearchBySim3(kf1, kf2, m, s12, cv::Mat(3, 3, cv::CV_32F, R12, 12), cv::Mat(3, 1, cv::CV_32F, t12, 4), th, z_as_written != 0);
    for (int i = 0; i < n1; ++i) matches12[i] = m[i];
    return nm;)
}
// The two Scw matchers of loop closing through the mirror.  The key frame: n key points with descriptors, map-point ids kf_mp (-1 = none; Fuse: in / out)
// and their bad flags or NULL; Scw 12 floats (rows 0..2 of [sR | t]); M points (position, normal, distance members, descriptor, id, bad flag or NULL).
// hm_search_by_projection_sim3: matched[n] = vpMatched as ids, in / out.  hm_fuse_sim3: replace[M] = vpReplacePoint as ids, in / out.
namespace {
void sim3p_views(KeyFrameView& kf, std::vector<MapPointView>& pts, int n, const cms_keypoint* k, const uint8_t* desc, const long* kf_mp, const uint8_t* kf_bad, int M,
                 const float* pos, const float* normal, const float* mn, const float* mx, const uint8_t* mpd, const long* mp_id, const uint8_t* mp_bad) {
  kf.mvKeys.resize(n);
  kf.mDescriptors.create(n > 0 ? n : 1, 32, cv::CV_8U);
  kf.mvpMapPoints.assign(kf_mp, kf_mp + n);
  if (kf_bad) kf.mvbMapPointBad.assign(kf_bad, kf_bad + n);
  for (int i = 0; i < n; ++i) {
    kf.mvKeys[i].pt = cv::Point2f(k[i].x, k[i].y); kf.mvKeys[i].angle = k[i].angle; kf.mvKeys[i].octave = k[i].octave; kf.mvKeys[i].size = k[i].size;
    kf.mvKeys[i].response = k[i].response;
    std::memcpy(kf.mDescriptors.ptr<uint8_t>(i), desc + (size_t)i * 32, 32);
  }
  pts.resize(M);
  for (int i = 0; i < M; ++i) {
    MapPointView& v = pts[i];
    v.mnId = mp_id[i]; v.mbBad = mp_bad && mp_bad[i]; v.mfMinDistance = mn[i]; v.mfMaxDistance = mx[i];
    v.mWorldPos.create(3, 1, cv::CV_32F); v.mNormalVector.create(3, 1, cv::CV_32F);
    for (int c = 0; c < 3; ++c) { v.mWorldPos.at<float>(c, 0) = pos[3 * (size_t)i + c]; v.mNormalVector.at<float>(c, 0) = normal[3 * (size_t)i + c]; }
    v.mDescriptor.create(1, 32, cv::CV_8U);
    std::memcpy(v.mDescriptor.ptr<uint8_t>(0), mpd + 32 * (size_t)i, 32);
  }
}
}  // namespace
extern "C" int hm_search_by_projection_sim3(int n, const cms_keypoint* k, const uint8_t* desc, float* Scw, int M, const float* pos, const float* normal, const float* mn,
                                            const float* mx, const uint8_t* mpd, const long* mp_id, const uint8_t* mp_bad, int th, long* matched) {
  HM_TRY(
    KeyFrameView kf;
    std::vector<MapPointView> pts;
    std::vector<long> none(n > 0 ? n : 1, -1);
    sim3p_views(kf, pts, n, k, desc, none.data(), nullptr, M, pos, normal, mn, mx, mpd, mp_id, mp_bad);
    std::vector<long> m(matched, matched + n);
    ORBMatcher matcher(0.75f, true);
    const int nm = matcher.SearchByProjection(kf, cv::Mat(3, 4, cv::CV_32F, Scw, 16), pts, m, th);
    for (int i = 0; i < n; ++i) matched[i] = m[i];
    return nm;)
}
extern "C" int hm_fuse_sim3(int n, const cms_keypoint* k, const uint8_t* desc, long* kf_mp, const uint8_t* kf_bad, float* Scw, int M, const float* pos, const float* normal,
                            const float* mn, const float* mx, const uint8_t* mpd, const long* mp_id, const uint8_t* mp_bad, float th, long* replace) {
  HM_TRY(
    KeyFrameView kf;
    std::vector<MapPointView> pts;
    sim3p_views(kf, pts, n, k, desc, kf_mp, kf_bad, M, pos, normal, mn, mx, mpd, mp_id, mp_bad);
    std::vector<long> r(replace, replace + M);
    ORBMatcher matcher(0.8f);
    const int nf = matcher.Fuse(kf, cv::Mat(3, 4, cv::CV_32F, Scw, 16), pts, th, r);
    for (int i = 0; i < M; ++i) replace[i] = r[i];
    for (int i = 0; i < n; ++i) kf_mp[i] = kf.mvpMapPoints[i];
    return nf;)
}
// LocalMapping::CreateNewMapPoints through the mirror: key frame 0 is the current one, 1..nkf-1 its neighbours.  Flat inputs:
// feat_off[nkf+1]; per feature kps/desc/rays/mp; Tcw nkf x 16; FeatureVector per key frame as node_off2[nkf+1] into (node_id, node_cnt)
// and the features of the nodes concatenated in node_feat; median_depth[nkf].  Outputs up to cap records.
extern "C" int hm_create_new_map_points(int nkf, const int* feat_off, const cms_keypoint* kps, const uint8_t* desc, const float* rays, const long* mp,
                                        float* Tcw, const int* node_off2, const int* node_id, const int* node_cnt, const int* node_feat,
                                        const float* median_depth, int cap, int* out_neigh, int* out_idx1, int* out_idx2, float* out_x3d) {
  HM_TRY(
    std::vector<KeyFrameView> kfs(nkf);
    size_t nf_cursor = 0;
    for (int k = 0; k < nkf; ++k) {
      KeyFrameView& v = kfs[k];
      const int f0 = feat_off[k], n = feat_off[k + 1] - f0;
      v.mnId = k; v.mvKeys.resize(n); v.mvKeyRays.resize(n); v.mvpMapPoints.assign(mp + f0, mp + f0 + n);
      v.mDescriptors.create(n > 0 ? n : 1, 32, cv::CV_8U);
      for (int i = 0; i < n; ++i) {
        const cms_keypoint& s = kps[f0 + i];
        v.mvKeys[i].pt = cv::Point2f(s.x, s.y); v.mvKeys[i].angle = s.angle; v.mvKeys[i].octave = s.octave;
        std::memcpy(v.mDescriptors.ptr<uint8_t>(i), desc + 32 * (size_t)(f0 + i), 32);
        for (int c = 0; c < 3; ++c) v.mvKeyRays[i].v[c] = rays[3 * (size_t)(f0 + i) + c];
      }
      v.Tcw = cv::Mat(4, 4, cv::CV_32F, Tcw + 16 * (size_t)k, 16);
      for (int e = node_off2[k]; e < node_off2[k + 1]; ++e) {
        std::vector<unsigned> fl(node_feat + nf_cursor, node_feat + nf_cursor + node_cnt[e]);
        nf_cursor += (size_t)node_cnt[e];
        v.mFeatVec.emplace_back((unsigned)node_id[e], std::move(fl));
      }
      v.medianDepth = median_depth[k];
    }
    std::vector<const KeyFrameView*> neigh;
    for (int k = 1; k < nkf; ++k) neigh.push_back(&kfs[k]);
    const std::vector<NewMapPoint> pts = LocalMapping::CreateNewMapPoints(kfs[0], neigh);
    const int n = (int)pts.size();
    for (int i = 0; i < n && i < cap; ++i) {
      out_neigh[i] = pts[i].neighbour; out_idx1[i] = pts[i].idx1; out_idx2[i] = pts[i].idx2;
      for (int c = 0; c < 3; ++c) out_x3d[3 * (size_t)i + c] = pts[i].x3D.v[c];
    }
    return n;)
}
// ORBMatcher::Fuse through the mirror (ORBMatcher.cpp:1127-1244): the key frame as flat arrays (n key points, descriptors, the map-point slot per key
// point: in / out), M map points (position, normal, distance range, descriptor, id), skip[M] (pMP->isBad() / IsInKeyFrame, may be NULL).  fused[M] = the
// key point every map point is fused with or -1; mp_slots receives the ADDITIONS (AddMapPoint for a free key point, in list order); for a key point
// that already holds a point the caller decides the Replace by Observations() like the reference does.  Returns nFused.
extern "C" int hm_fuse(int n, const cms_keypoint* kps, const uint8_t* desc, long* mp_slots, float* Tcw, int M, const float* pos, const float* normal,
                       const float* min_dist, const float* max_dist, const uint8_t* mp_desc, const long* mp_id, const uint8_t* skip, float th, int* fused) {
  HM_TRY(
    KeyFrameView v;
    v.mnId = 0; v.mvKeys.resize(n); v.mvpMapPoints.assign(mp_slots, mp_slots + n);
    v.mDescriptors.create(n > 0 ? n : 1, 32, cv::CV_8U);
    for (int i = 0; i < n; ++i) {
      v.mvKeys[i].pt = cv::Point2f(kps[i].x, kps[i].y); v.mvKeys[i].angle = kps[i].angle; v.mvKeys[i].octave = kps[i].octave;
      v.mvKeys[i].size = kps[i].size; v.mvKeys[i].response = kps[i].response;
      std::memcpy(v.mDescriptors.ptr<uint8_t>(i), desc + 32 * (size_t)i, 32);
    }
    v.Tcw = cv::Mat(4, 4, cv::CV_32F, Tcw, 16);
    std::vector<MapPointView> mps(M);
    std::vector<float> store(6 * (size_t)std::max(M, 1));
    std::vector<uint8_t> dstore(32 * (size_t)std::max(M, 1));
    for (int i = 0; i < M; ++i) {
      for (int c = 0; c < 3; ++c) { store[6 * (size_t)i + c] = pos[3 * (size_t)i + c]; store[6 * (size_t)i + 3 + c] = normal[3 * (size_t)i + c]; }
      std::memcpy(&dstore[32 * (size_t)i], mp_desc + 32 * (size_t)i, 32);
      mps[i].mnId = mp_id[i];
      mps[i].mWorldPos = cv::Mat(3, 1, cv::CV_32F, &store[6 * (size_t)i], 4);
      mps[i].mNormalVector = cv::Mat(3, 1, cv::CV_32F, &store[6 * (size_t)i + 3], 4);
      mps[i].mfMinDistance = min_dist[i]; mps[i].mfMaxDistance = max_dist[i];
      mps[i].mDescriptor = cv::Mat(1, 32, cv::CV_8U, &dstore[32 * (size_t)i], 32);
    }
    std::vector<uint8_t> sk;
    if (skip) sk.assign(skip, skip + M);
    std::vector<int> f;
    ORBMatcher matcher;
    const int nf = matcher.Fuse(v, mps, sk, th, f);
    for (int i = 0; i < M; ++i) fused[i] = f[i];
    for (int i = 0; i < n; ++i) mp_slots[i] = v.mvpMapPoints[i];
    return nf;)
}
// local BA through the Optimizer mirror.  Tcw: K x 16 float (row major 4x4), Xw: P x 3 float, observations flat.
extern "C" int hm_local_ba(int K, float* Tcw, const long* kf_id, const uint8_t* kf_fixed, const float* inv_sigma2, int nlevels, int P,
                           float* Xw, int nobs, const int* obs_kf, const int* obs_mp, const cms_keypoint* obs_kp, const float* obs_ray,
                           uint8_t* stop, int* erase_pairs, int erase_cap) {
  HM_TRY(
    LocalBAWindow w;
    w.keyframes.resize(K);
    for (int k = 0; k < K; ++k) {
      w.keyframes[k].mnId = kf_id[k]; w.keyframes[k].fixed = kf_fixed[k] != 0;
      w.keyframes[k].Tcw = cv::Mat(4, 4, cv::CV_32F, Tcw + 16 * (size_t)k, 16);
      w.keyframes[k].mvInvLevelSigma2.assign(inv_sigma2, inv_sigma2 + nlevels);
    }
    w.mappoints.resize(P);
    for (int p = 0; p < P; ++p) { w.mappoints[p].mnId = p; w.mappoints[p].Xw = cv::Mat(3, 1, cv::CV_32F, Xw + 3 * (size_t)p, 4); }
    for (int o = 0; o < nobs; ++o) {
      LocalBAWindow::Obs ob;
      ob.kf = obs_kf[o];
      ob.kp.pt = cv::Point2f(obs_kp[o].x, obs_kp[o].y); ob.kp.octave = obs_kp[o].octave;
      ob.ray.v[0] = obs_ray[3 * o]; ob.ray.v[1] = obs_ray[3 * o + 1]; ob.ray.v[2] = obs_ray[3 * o + 2];
      w.mappoints[obs_mp[o]].observations.push_back(ob);
    }
    Optimizer::LocalBundleAdjustment(&w, reinterpret_cast<bool*>(stop));
    const int n = (int)w.toErase.size();
    for (int i = 0; i < n && i < erase_cap; ++i) { erase_pairs[2 * i] = w.toErase[i].first; erase_pairs[2 * i + 1] = w.toErase[i].second; }
    return n;)
}

// Optimizer::PoseOptimization on a Frame given as flat arrays: Tcw 4x4 float in/out, N key points (x, y, octave), rays N x 3,
// has_mp N, Xw N x 3 (float), inv_sigma2[nlevels]; outlier N out.  Returns the reference's return value.
extern "C" int hm_pose_optimization(float* Tcw, int N, const cms_keypoint* kps, const float* rays, const uint8_t* has_mp, const float* Xw,
                                    const float* inv_sigma2, int nlevels, uint8_t* outlier) {
  HM_TRY(
    PoseFrame fr;
    fr.mTcw = cv::Mat(4, 4, cv::CV_32F, Tcw, 16);
    fr.N = N;
    fr.mvKeys.resize(N); fr.mvKeyRays.resize(N); fr.mvbHasMapPoint.resize(N); fr.mvMapPointPos.resize(N);
    for (int i = 0; i < N; ++i) {
      fr.mvKeys[i].pt = cv::Point2f(kps[i].x, kps[i].y); fr.mvKeys[i].octave = kps[i].octave;
      for (int k = 0; k < 3; ++k) { fr.mvKeyRays[i].v[k] = rays[3 * i + k]; fr.mvMapPointPos[i].v[k] = Xw[3 * i + k]; }
      fr.mvbHasMapPoint[i] = has_mp[i] != 0;
    }
    fr.mvInvLevelSigma2.assign(inv_sigma2, inv_sigma2 + nlevels);
    const int r = Optimizer::PoseOptimization(&fr);
    for (int i = 0; i < N; ++i) outlier[i] = (i < (int)fr.mvbOutlier.size() && fr.mvbOutlier[i]) ? 1 : 0;
    return r;)
}

// System::SaveKeyFrameTrajectoryTUM on n key frames given as time stamps + 4x4 float Tcw
extern "C" int hm_save_trajectory_tum(const char* path, int n, const double* ts, float* Tcw) {
  HM_TRY(
    std::vector<TrajectoryKeyFrame> v(n);
    for (int i = 0; i < n; ++i) { v[i].mTimeStamp = ts[i]; v[i].Tcw = cv::Mat(4, 4, cv::CV_32F, Tcw + 16 * (size_t)i, 16); }
    System::SaveKeyFrameTrajectoryTUM(path, v);
    return n;)
}

// ---- file formats (io_formats.h); host only, usable without a GPU
extern "C" int hm_settings_load(const char* path, cms_camera* cam, cms_orb_params* orb, float* fps, int* with_mask, int* rgb) {
  HM_TRY(
    Settings st;
    if (!st.Load(path)) throw std::runtime_error(std::string("Failed to open settings file at: ") + path);
    if (cam) *cam = st.Camera();
    if (orb) *orb = st.Orb();
    if (fps) *fps = st.Fps();
    if (with_mask) *with_mask = st.WithFisheyeMask();
    if (rgb) *rgb = st.RGB() ? 1 : 0;
    return 0;)
}
// kind 0 = Lafida list, 1 = Fangshan list.  names: cap x name_len chars (NUL terminated).  Returns the number of entries.
extern "C" int hm_load_image_list(const char* path, int kind, int cap, int name_len, char* names, double* timestamps) {
  HM_TRY(
    const ImageList l = kind == 0 ? LoadImageListLafida(path) : LoadImageListFangshan(path);
    const int n = (int)l.names.size();
    for (int i = 0; i < n && i < cap; ++i) {
      std::strncpy(names + (size_t)i * name_len, l.names[i].c_str(), name_len - 1);
      names[(size_t)i * name_len + name_len - 1] = 0;
      timestamps[i] = l.timestamps[i];
    }
    return n;)
}
extern "C" int hm_write_tracking_summary(const char* path, float* times, int n, int frame_counter, char* console, int console_len) {
  HM_TRY(
    std::vector<float> v(times, times + n);
    const std::string text = WriteTrackingSummary(path ? path : "", v, frame_counter);
    std::copy(v.begin(), v.end(), times);
    if (console && console_len > 0) { std::strncpy(console, text.c_str(), console_len - 1); console[console_len - 1] = 0; }
    return 0;)
}

// PnPsolver through the mirror: n key points (kps, rays), the matched map point per key point (mp < 0 = none, bad, pos), the pyramid's sigma2.
// draws: the values the replaceable draw function hands out in order (it must not run dry).  Outputs: key_idx[N] = mvKeyPointIndices (returns N through
// *N_out), vb[n] = vbInliers (all zero when empty), Tcw16, state[4] = bNoMore, nInliers, mnIterations, found; returns 0, or -1 with hm_last_error().
extern "C" int hm_pnp_mirror(int engine, int n, const cms_keypoint* kps, const float* rays, const long* mp, const uint8_t* bad, const float* pos, int nlevels,
                             const float* sigma2, double probability, int minInliers, int maxIterations, float epsilon, float th2, int calls, const int* nIterations,
                             int n_draws, const int* draws, int* N_out, int* key_idx, uint8_t* vb, float* Tcw16, int* state) {
  HM_TRY(
    FrameView f;
    f.mvKeys.resize(n); f.mvKeyRays.resize(n); f.mvMapPointPos.resize(n);
    for (int i = 0; i < n; ++i) {
      f.mvKeys[i].pt = cv::Point2f(kps[i].x, kps[i].y); f.mvKeys[i].octave = kps[i].octave;
      for (int c = 0; c < 3; ++c) { f.mvKeyRays[i](c) = rays[3 * (size_t)i + c]; f.mvMapPointPos[i](c) = pos[3 * (size_t)i + c]; }
    }
    f.mvLevelSigma2.assign(sigma2, sigma2 + nlevels);
    if (bad) f.mvbMapPointBad.assign(bad, bad + n);
    PnPsolver solver(f, std::vector<long>(mp, mp + n));
    solver.engine = engine ? PnPsolver::HOST_CORE : PnPsolver::DEVICE;
    solver.SetRansacParameters(probability, minInliers, maxIterations, 4, epsilon, th2);
    int next = 0;
    solver.draw = [&](int lo, int hi) { if (next >= n_draws) throw std::runtime_error("hm_pnp_mirror: out of draws"); const int v = draws[next++]; if (v < lo || v > hi) throw std::runtime_error("hm_pnp_mirror: draw out of range"); return v; };
    *N_out = solver.N;
    for (int i = 0; i < solver.N; ++i) key_idx[i] = (int)solver.mvKeyPointIndices[i];
    std::vector<bool> vbInliers; int nInliers = 0; bool bNoMore = false; cv::Mat T;
    for (int c = 0; c < calls; ++c) {
      T = solver.iterate(nIterations[c], bNoMore, vbInliers, nInliers);
      if (!T.empty() || bNoMore) break;
    }
    std::memset(vb, 0, n);
    for (size_t i = 0; i < vbInliers.size(); ++i) vb[i] = vbInliers[i] ? 1 : 0;
    std::memset(Tcw16, 0, 64);
    if (!T.empty()) for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) Tcw16[4 * r + c] = T.at<float>(r, c);
    state[0] = bNoMore; state[1] = nInliers; state[2] = solver.mnIterations; state[3] = T.empty() ? 0 : 1; state[4] = next;
    return 0;)
}

// Sim3Solver through the mirror.  Per key frame k = 1, 2: Tcw (3 x 4: Rcw | tcw), sigma2 (nlevels), octave (nk key points), pos (np map points x 3), bad
// and index_in_kf (np).  mp1[nk1] = GetMapPointMatches() of key frame 1 as indices into its map points, matched12[n1] = indices into key frame 2's.
// draws: the values the replaceable draw function hands out in order (it must not run dry).  Outputs: idx1[N] = mvnIndices1 (N through *N_out),
// x12[N x 6] = mvX3Dc1 | mvX3Dc2, vb[n1] = vbInliers, T16 (zeros when empty), Rts[13] = GetEstimatedRotation | Translation | Scale, state[6] =
// bNoMore, nInliers, mnIterations, found, draws used, mRansacMaxIts; returns 0, or -1 with hm_last_error().
extern "C" int hm_sim3_mirror(int engine, int n1, int nk1, int nk2, int nlevels, int np1, int np2, const float* Tcw1, const float* sigma2_1, const int* octave1,
                              const float* pos1, const uint8_t* bad1, const int* index1, const float* Tcw2, const float* sigma2_2, const int* octave2, const float* pos2,
                              const uint8_t* bad2, const int* index2, const int* mp1, const int* matched12, int fix_scale, double probability, int minInliers,
                              int maxIterations, int calls, const int* nIterations, int n_draws, const int* draws, int* N_out, int* idx1, float* x12, uint8_t* vb,
                              float* T16, float* Rts, int* state) {
  HM_TRY(
    auto fill = [&](Sim3KeyFrameView& k, int nk, int np, const float* Tcw, const float* sigma2, const int* octave, const float* pos, const uint8_t* bad, const int* index) {
      for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) k.Rcw[3 * r + c] = Tcw[4 * r + c]; k.tcw[r] = Tcw[4 * r + 3]; }
      k.mvLevelSigma2.assign(sigma2, sigma2 + nlevels);
      k.mvKeyOctaves.assign(octave, octave + nk);
      k.mvMapPoints.resize(np);
      for (int i = 0; i < np; ++i) {
        for (int c = 0; c < 3; ++c) k.mvMapPoints[i].mWorldPos(c) = pos[3 * (size_t)i + c];
        k.mvMapPoints[i].mbBad = bad[i] != 0; k.mvMapPoints[i].mnIndexInKeyFrame = index[i];
      }
    };
    Sim3KeyFrameView k1; Sim3KeyFrameView k2;
    fill(k1, nk1, np1, Tcw1, sigma2_1, octave1, pos1, bad1, index1);
    fill(k2, nk2, np2, Tcw2, sigma2_2, octave2, pos2, bad2, index2);
    k1.mvpMapPointMatches.assign(mp1, mp1 + nk1);
    Sim3Solver solver(k1, k2, std::vector<int>(matched12, matched12 + n1), fix_scale != 0);
    solver.engine = engine ? Sim3Solver::HOST_CORE : Sim3Solver::DEVICE;
    solver.SetRansacParameters(probability, minInliers, maxIterations);
    int next = 0;
    solver.draw = [&](int lo, int hi) { if (next >= n_draws) throw std::runtime_error("hm_sim3_mirror: out of draws"); const int v = draws[next++]; if (v < lo || v > hi) throw std::runtime_error("hm_sim3_mirror: draw out of range"); return v; };
    *N_out = solver.N;
    for (int i = 0; i < solver.N; ++i) {
      idx1[i] = (int)solver.mvnIndices1[i];
      for (int c = 0; c < 3; ++c) { x12[6 * (size_t)i + c] = solver.mvX3Dc1[i](c); x12[6 * (size_t)i + 3 + c] = solver.mvX3Dc2[i](c); }
    }
    std::vector<bool> vbInliers; int nInliers = 0; bool bNoMore = false; cv::Mat T;
    for (int c = 0; c < calls; ++c) {
      T = solver.iterate(nIterations[c], bNoMore, vbInliers, nInliers);
      if (!T.empty() || bNoMore) break;
    }
    std::memset(vb, 0, n1);
    for (size_t i = 0; i < vbInliers.size(); ++i) vb[i] = vbInliers[i] ? 1 : 0;
    std::memset(T16, 0, 64);
    if (!T.empty()) for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T16[4 * r + c] = T.at<float>(r, c);
    cv::Mat R = solver.GetEstimatedRotation(); cv::Mat t = solver.GetEstimatedTranslation();
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) Rts[3 * r + c] = R.at<float>(r, c); Rts[9 + r] = t.at<float>(r, 0); }
    Rts[12] = solver.GetEstimatedScale();
    state[0] = bNoMore; state[1] = nInliers; state[2] = solver.mnIterations; state[3] = T.empty() ? 0 : 1; state[4] = next; state[5] = solver.mRansacMaxIts;
    return 0;)
}

// Optimizer::OptimizeSim3 through the mirror.  Per key frame k = 1, 2: Tcw (3 x 4: Rcw | tcw), inv_sigma2 (nlevels), octave and kpts (nk key points, x y),
// pos / bad / index_in_kf (np map points).  mp1[nk1] = GetMapPointMatches() of key frame 1, matches1[n1] in/out = vpMatches1 as indices into key frame
// 2's map points (-1 = NULL).  S12[13] = R | t | s in.  Outputs: *N_out and idx[N] = vnIndexEdge, x12[N x 6] = P3D1c | P3D2c, kp12[N x 4] = kp1 | kp2,
// is12[N x 2] = both invSigma2 (room for n1 pairs each), out8 = q (x y z w) | t | s, *n_inliers.  Returns 0, or -1 with hm_last_error().
extern "C" int hm_sim3_opt_mirror(int engine, int jacobian, int n1, int nk1, int nk2, int nlevels, int np1, int np2, const float* Tcw1, const float* inv_sigma2_1,
                                  const int* octave1, const float* kpts1, const float* pos1, const uint8_t* bad1, const int* index1, const float* Tcw2,
                                  const float* inv_sigma2_2, const int* octave2, const float* kpts2, const float* pos2, const uint8_t* bad2, const int* index2,
                                  const int* mp1, int* matches1, const double* S12, float th2, int fix_scale, int* N_out, int* idx, float* x12, float* kp12, float* is12,
                                  double* out8, int* n_inliers) {
  HM_TRY(
    auto fill = [&](Sim3OptKeyFrameView& k, int nk, int np, const float* Tcw, const float* inv, const int* octave, const float* kpts, const float* pos, const uint8_t* bad,
                    const int* index) {
      for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) k.Rcw[3 * r + c] = Tcw[4 * r + c]; k.tcw[r] = Tcw[4 * r + 3]; }
      k.mvInvLevelSigma2.assign(inv, inv + nlevels);
      k.mvKeyOctaves.assign(octave, octave + nk);
      k.mvKeyPts.resize(nk);
      for (int i = 0; i < nk; ++i) k.mvKeyPts[i] = cv::Point2f(kpts[2 * (size_t)i], kpts[2 * (size_t)i + 1]);
      k.mvMapPoints.resize(np);
      for (int i = 0; i < np; ++i) {
        for (int c = 0; c < 3; ++c) k.mvMapPoints[i].mWorldPos(c) = pos[3 * (size_t)i + c];
        k.mvMapPoints[i].mbBad = bad[i] != 0; k.mvMapPoints[i].mnIndexInKeyFrame = index[i];
      }
    };
    Sim3OptKeyFrameView k1; Sim3OptKeyFrameView k2;
    fill(k1, nk1, np1, Tcw1, inv_sigma2_1, octave1, kpts1, pos1, bad1, index1);
    fill(k2, nk2, np2, Tcw2, inv_sigma2_2, octave2, kpts2, pos2, bad2, index2);
    k1.mvpMapPointMatches.assign(mp1, mp1 + nk1);
    std::vector<int> vpMatches1(matches1, matches1 + n1);
    const Sim3OptGraph g = Optimizer::CollectSim3Graph(k1, k2, vpMatches1);
    const int N = (int)g.vnIndexEdge.size();
    *N_out = N;
    for (int k = 0; k < N; ++k) {
      idx[k] = (int)g.vnIndexEdge[(size_t)k];
      for (int c = 0; c < 3; ++c) { x12[6 * (size_t)k + c] = g.x3dc1[3 * (size_t)k + c]; x12[6 * (size_t)k + 3 + c] = g.x3dc2[3 * (size_t)k + c]; }
      for (int c = 0; c < 2; ++c) { kp12[4 * (size_t)k + c] = g.kp1[2 * (size_t)k + c]; kp12[4 * (size_t)k + 2 + c] = g.kp2[2 * (size_t)k + c]; }
      is12[2 * (size_t)k] = g.invSigma2_1[(size_t)k]; is12[2 * (size_t)k + 1] = g.invSigma2_2[(size_t)k];
    }
    Sim3Value S;
    std::memcpy(S.R, S12, 72); std::memcpy(S.t, S12 + 9, 24); S.s = S12[12];
    *n_inliers = Optimizer::OptimizeSim3(k1, k2, vpMatches1, S, th2, fix_scale != 0, engine ? Optimizer::HOST_CORE : Optimizer::DEVICE, jacobian);
    std::memcpy(matches1, vpMatches1.data(), sizeof(int) * (size_t)n1);
    std::memcpy(out8, S.q, 32); std::memcpy(out8 + 4, S.t, 24); out8[7] = S.s;
    return 0;)
}

// Initializer through the mirror: the reference frame (n1 key points, rays) and the current frame (n2), vMatches12 (n1).  draws: the values the
// replaceable draw function hands out in order (it must not run dry; n_draws < 0 keeps the class's default draw).  vP3D / vbTriangulated go in holding the caller's pattern, so that "left as they
// were" shows.  Outputs: R21 (9, zeros when empty), t21 (3), p3d (3 per entry of vP3D), tri, sets[8 * iterations] = mvSets, state[0..11] = found, draws
// used, N, vP3D.size(), vbTriangulated.size(), best iteration, inliers, winner, nGood[4]; diag[0..4] = score, parallax[4].  Returns 0, or -1 with
// hm_last_error().
extern "C" int hm_init_mirror(int engine, int n1, const cms_keypoint* kps1, const float* rays1, int n2, const cms_keypoint* kps2, const float* rays2,
                              const int* matches12, float sigma, int iterations, int n_draws, const int* draws, float* R21, float* t21, int p3d_len, float* p3d,
                              int tri_len, uint8_t* tri, int* sets, int* state, float* diag) {
  HM_TRY(
    FrameView f1, f2;
    f1.mvKeys.resize(n1); f1.mvKeyRays.resize(n1); f2.mvKeys.resize(n2); f2.mvKeyRays.resize(n2);
    for (int i = 0; i < n1; ++i) { f1.mvKeys[i].pt = cv::Point2f(kps1[i].x, kps1[i].y); for (int c = 0; c < 3; ++c) f1.mvKeyRays[i](c) = rays1[3 * (size_t)i + c]; }
    for (int i = 0; i < n2; ++i) { f2.mvKeys[i].pt = cv::Point2f(kps2[i].x, kps2[i].y); for (int c = 0; c < 3; ++c) f2.mvKeyRays[i](c) = rays2[3 * (size_t)i + c]; }
    Initializer ini(f1, sigma, iterations);
    ini.engine = engine ? Initializer::HOST_CORE : Initializer::DEVICE;
    int next = 0;
    if (n_draws >= 0) ini.draw = [&](int lo, int hi) { if (next >= n_draws) throw std::runtime_error("hm_init_mirror: out of draws"); const int v = draws[next++]; if (v < lo || v > hi) throw std::runtime_error("hm_init_mirror: draw out of range"); return v; };
    std::vector<cv::Point3f> vP3D((size_t)p3d_len);
    std::vector<bool> vbTriangulated((size_t)tri_len);
    for (int i = 0; i < p3d_len; ++i) vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
    for (int i = 0; i < tri_len; ++i) vbTriangulated[i] = tri[i] != 0;
    cv::Mat R, t;
    const bool found = ini.InitializeWithRays(f2, std::vector<int>(matches12, matches12 + n1), R, t, vP3D, vbTriangulated);
    for (int k = 0; k < 9; ++k) R21[k] = R.empty() ? 0.0f : R.at<float>(k / 3, k % 3);
    for (int k = 0; k < 3; ++k) t21[k] = t.empty() ? 0.0f : t.at<float>(k, 0);
    for (size_t i = 0; i < vP3D.size() && (int)i < std::max(p3d_len, n1); ++i) { p3d[3 * i] = vP3D[i].x; p3d[3 * i + 1] = vP3D[i].y; p3d[3 * i + 2] = vP3D[i].z; }
    for (size_t i = 0; i < vbTriangulated.size() && (int)i < std::max(tri_len, n1); ++i) tri[i] = vbTriangulated[i] ? 1 : 0;
    for (size_t it = 0; it < ini.mvSets.size() && (int)it < iterations; ++it)
      for (int k = 0; k < 8; ++k) sets[8 * it + k] = (int)ini.mvSets[it][k];
    state[0] = found; state[1] = next; state[2] = (int)ini.mvMatches12.size(); state[3] = (int)vP3D.size(); state[4] = (int)vbTriangulated.size();
    state[5] = ini.mnBestIteration; state[6] = ini.mnInliers; state[7] = ini.mnWinner;
    for (int h = 0; h < 4; ++h) { state[8 + h] = ini.mnGood[h]; diag[1 + h] = ini.mfParallax[h]; }
    diag[0] = ini.mfScore;
    return 0;)
}

// ---- ORBVocabulary (tests/vocab_hostlib.py): the mirror class, the text format and the host build of csrc/cms_vocab_core.h
extern "C" int hm_vocab_create(void** out, int k, int L, int scoring, int weighting, int n_nodes, const int* parent, const uint8_t* is_leaf, const uint8_t* desc,
                               const double* weight) {
  HM_TRY(
    if (n_nodes < 1) throw std::runtime_error("vocabulary: no nodes");
    VocabularyText t;
    t.k = k; t.L = L; t.scoring = scoring; t.weighting = weighting;
    t.parent.assign(parent, parent + n_nodes); t.is_leaf.assign(is_leaf, is_leaf + n_nodes); t.desc.assign(desc, desc + 32 * (size_t)n_nodes);
    t.weight.assign(weight, weight + n_nodes);
    ORBVocabulary* v = new ORBVocabulary();
    if (!v->setTree(t)) { const std::string why = v->error(); delete v; throw std::runtime_error(why); }
    *out = v;
    return 0;)
}
extern "C" int hm_vocab_load(void** out, const char* path) {
  HM_TRY(
    ORBVocabulary* v = new ORBVocabulary();
    if (!v->loadFromTextFile(path)) { const std::string why = v->error(); delete v; throw std::runtime_error(why); }
    *out = v;
    return 0;)
}
extern "C" int hm_vocab_save(void* voc, const char* path) {
  HM_TRY(static_cast<ORBVocabulary*>(voc)->saveToTextFile(path); return 0;)
}
extern "C" void hm_vocab_destroy(void* voc) { delete static_cast<ORBVocabulary*>(voc); }
// info[6]: k, L, scoring, weighting, nodes, words
extern "C" int hm_vocab_info(void* voc, int* info) {
  HM_TRY(
    const ORBVocabulary* v = static_cast<ORBVocabulary*>(voc);
    const VocabularyText& t = v->tree();
    info[0] = t.k; info[1] = t.L; info[2] = t.scoring; info[3] = t.weighting; info[4] = t.nodes(); info[5] = (int)v->size();
    return 0;)
}
extern "C" int hm_vocab_arrays(void* voc, int* parent, uint8_t* is_leaf, uint8_t* desc, double* weight) {
  HM_TRY(
    const VocabularyText& t = static_cast<ORBVocabulary*>(voc)->tree();
    std::memcpy(parent, t.parent.data(), 4 * t.parent.size()); std::memcpy(is_leaf, t.is_leaf.data(), t.is_leaf.size());
    std::memcpy(desc, t.desc.data(), t.desc.size()); std::memcpy(weight, t.weight.data(), 8 * t.weight.size());
    return 0;)
}
// ORBVocabulary::transform through the named engine (0 = device, 1 = host core); arrays of n entries, node_off n + 1
extern "C" int hm_vocab_transform(void* voc, int engine, int n, const uint8_t* desc, int levelsup, int* nwords, int* word_id, double* word_val, int* nnodes,
                                  int* node_id, int* node_off, int* node_feat) {
  HM_TRY(
    ORBVocabulary* v = static_cast<ORBVocabulary*>(voc);
    v->engine = engine ? ORBVocabulary::HOST_CORE : ORBVocabulary::DEVICE;
    std::vector<cv::Mat> feats((size_t)n);
    for (int i = 0; i < n; ++i) feats[(size_t)i] = cv::Mat(1, 32, cv::CV_8U, const_cast<uint8_t*>(desc) + 32 * (size_t)i, 32);
    BowVector bv;
    FeatureVector fv;
    v->transform(feats, bv, fv, levelsup);
    *nwords = (int)bv.size(); *nnodes = (int)fv.size();
    for (size_t i = 0; i < bv.size(); ++i) { word_id[i] = (int)bv[i].first; word_val[i] = bv[i].second; }
    int at = 0;
    node_off[0] = 0;
    for (size_t e = 0; e < fv.size(); ++e) {
      node_id[e] = (int)fv[e].first;
      for (unsigned f : fv[e].second) node_feat[at++] = (int)f;
      node_off[e + 1] = at;
    }
    return 0;)
}
// Frame::ComputeBoW (keyframe == 0) / KeyFrame::ComputeBoW (keyframe != 0) through the host core with mBowVec / mFeatVec holding a marker entry
// beforehand when pre_bow / pre_fv say so: out[0] = 1 when the vectors were recomputed, out[1] / out[2] = their sizes afterwards
extern "C" int hm_vocab_compute_bow_guard(void* voc, int keyframe, int n, const uint8_t* desc, int pre_bow, int pre_fv, int* out) {
  HM_TRY(
    ORBVocabulary* v = static_cast<ORBVocabulary*>(voc);
    v->engine = ORBVocabulary::HOST_CORE;
    cv::Mat D(std::max(n, 1), 32, cv::CV_8U, const_cast<uint8_t*>(desc), 32);
    if (n == 0) D.rows = 0;
    const unsigned marker = 0xFFFFFFFFu;
    BowVector bv;
    FeatureVector fv;
    if (pre_bow) bv.push_back(std::make_pair(marker, -1.0));
    if (pre_fv) fv.push_back(std::make_pair(marker, std::vector<unsigned>()));
    if (keyframe) { KeyFrameView k; k.mDescriptors = D; k.mBowVec = bv; k.mFeatVec = fv; k.ComputeBoW(*v); bv = k.mBowVec; fv = k.mFeatVec; }
    else { FrameView f; f.mDescriptors = D; f.mBowVec = bv; f.mFeatVec = fv; f.ComputeBoW(*v); bv = f.mBowVec; fv = f.mFeatVec; }
    const bool kept = (pre_bow && !bv.empty() && bv[0].first == marker) || (pre_fv && !fv.empty() && fv[0].first == marker);
    out[0] = kept ? 0 : 1; out[1] = (int)bv.size(); out[2] = (int)fv.size();
    return 0;)
}
extern "C" int hm_vocab_score(void* voc, int n1, const int* id1, const double* val1, int n2, const int* id2, const double* val2, double* out) {
  HM_TRY(
    BowVector a, b;
    for (int i = 0; i < n1; ++i) a.push_back(std::make_pair((unsigned)id1[i], val1[i]));
    for (int i = 0; i < n2; ++i) b.push_back(std::make_pair((unsigned)id2[i], val2[i]));
    *out = static_cast<ORBVocabulary*>(voc)->score(a, b);
    return 0;)
}
// the core's single-descriptor descent, feature by feature: word id, node id and the word's weight
extern "C" int hm_vocab_descend(void* voc, int n, const uint8_t* desc, int levelsup, int* word, int* nid, double* weight) {
  HM_TRY(
    const VocabularyText& t = static_cast<ORBVocabulary*>(voc)->tree();
    CmsVocabTree tree;
    const char* why = cms_vocab_relayout(t.k, t.L, t.scoring, t.weighting, t.nodes(), t.parent.data(), t.is_leaf.data(), t.desc.data(), t.weight.data(), &tree);
    if (why) throw std::runtime_error(why);
    const CmsVocabView view = tree.view();
    for (int i = 0; i < n; ++i) {
      uint32_t f[8];
      std::memcpy(f, desc + 32 * (size_t)i, 32);
      int leaf;
      cms_vocab_descend(view, f, levelsup, &word[i], &nid[i], &leaf);
      weight[i] = view.word_weight[word[i]];
    }
    return 0;)
}

// ---- KeyFrameDatabase (tests/kfdb_hostlib.py): the host build of csrc/cms_kfdb_core.h, the definition of record of cms_kfdb_detect.  The calls mirror
// the C-ABI's (cms_kfstore_set_bow, cms_kfdb_*) on a handle of its own; they return 0, -1 (CMS_ERR_ARG, nothing changed) or -4 (CMS_ERR_OVERFLOW).
extern "C" int hm_kfdb_create(void** out, int max_keyframes, int max_features) {
  HM_TRY(
    if (!out || max_keyframes < 1 || max_features < 1) throw std::runtime_error("hm_kfdb_create: bad argument");
    *out = new CmsKfdbHost(max_keyframes, max_features);
    return 0;)
}
extern "C" void hm_kfdb_destroy(void* db) { delete static_cast<CmsKfdbHost*>(db); }
extern "C" int hm_kfdb_set_bow(void* db, int slot, int nwords, const int* word_id, const double* word_val) {
  CmsKfdbHost* d = static_cast<CmsKfdbHost*>(db);
  if (d->slot_ok(slot) && d->slots[(size_t)slot].in_db) return -1;
  return d->set_bow(slot, nwords, word_id, word_val);
}
// what cms_kfstore_put* does to the slot's BowVector and its database entry
extern "C" int hm_kfdb_refill(void* db, int slot) {
  CmsKfdbHost* d = static_cast<CmsKfdbHost*>(db);
  if (!d->slot_ok(slot)) return -1;
  d->refill(slot);
  return 0;
}
extern "C" int hm_kfdb_add(void* db, int n, const int* slots, const int* groups) { return static_cast<CmsKfdbHost*>(db)->add(n, slots, groups); }
extern "C" int hm_kfdb_erase(void* db, int n, const int* slots) { return static_cast<CmsKfdbHost*>(db)->erase(n, slots); }
extern "C" int hm_kfdb_clear(void* db, int group) { static_cast<CmsKfdbHost*>(db)->clear(group); return 0; }
extern "C" int hm_kfdb_set_covisibles(void* db, int n, const int* slots, const int* neigh) { return static_cast<CmsKfdbHost*>(db)->set_covisibles(n, slots, neigh); }
// cms_kfdb_detect's arguments; a job names a slot (CMS_KFDB_QUERY_SLOT) or carries its words (CMS_KFDB_QUERY_WORDS): there are no frame rows here
extern "C" int hm_kfdb_detect(void* db, int njobs, const cms_kfdb_job* jobs, int cand_cap, int* cand_slot, int* n_cand, int* diag_common, float* diag_score) {
  HM_TRY(
    CmsKfdbHost* d = static_cast<CmsKfdbHost*>(db);
    const size_t K = d->slots.size();
    for (int j = 0; j < njobs; ++j) {
      const cms_kfdb_job& q = jobs[j];
      if ((q.mode != CMS_KFDB_RELOC && q.mode != CMS_KFDB_LOOP) || q.group < 0) return -1;
      if (q.query == CMS_KFDB_QUERY_SLOT) { if (!d->slot_ok(q.slot) || !d->slots[(size_t)q.slot].has_bow) return -1; }
      else if (q.query == CMS_KFDB_QUERY_WORDS) { if (q.nwords < 0 || !cms_kfdb_bow_ok(q.nwords, q.word_id)) return -1; }
      else return -1;
      if (q.mode == CMS_KFDB_LOOP)
        for (int i = 0; i < q.n_connected; ++i) if (!d->slot_ok(q.connected[i])) return -1;
    }
    bool overflow = false;
    for (int j = 0; j < njobs; ++j) {
      const cms_kfdb_job& q = jobs[j];
      CmsKfdbQuery hq;
      hq.mode = q.mode; hq.group = q.group; hq.min_score = q.min_score; hq.n_connected = q.mode == CMS_KFDB_LOOP ? q.n_connected : 0; hq.connected = q.connected;
      hq.bow = q.query == CMS_KFDB_QUERY_SLOT ? d->bow(q.slot) : CmsKfdbBow{q.nwords, q.word_id, q.word_val};
      std::vector<int> cand;
      d->detect(hq, &cand, diag_common ? diag_common + (size_t)j * K : nullptr, diag_score ? diag_score + (size_t)j * K : nullptr);
      n_cand[j] = (int)cand.size();
      if ((int)cand.size() > cand_cap) overflow = true;
      for (int i = 0; i < std::min((int)cand.size(), cand_cap); ++i) cand_slot[(size_t)j * cand_cap + i] = cand[(size_t)i];
    }
    return overflow ? -4 : 0;)
}
extern "C" int hm_kfdb_bow_score(void* db, int npairs, const int* slot_a, const int* slot_b, double* score) {
  CmsKfdbHost* d = static_cast<CmsKfdbHost*>(db);
  for (int i = 0; i < npairs; ++i)
    if (!d->slot_ok(slot_a[i]) || !d->slot_ok(slot_b[i]) || !d->slots[(size_t)slot_a[i]].has_bow || !d->slots[(size_t)slot_b[i]].has_bow) return -1;
  for (int i = 0; i < npairs; ++i) score[i] = cms_kfdb_score_host(d->bow(slot_a[i]), d->bow(slot_b[i]));
  return 0;
}
// the core's score of two BowVectors (against ORBVocabulary::score: hm_vocab_score)
extern "C" int hm_kfdb_score(int n1, const int* id1, const double* val1, int n2, const int* id2, const double* val2, double* out) {
  *out = cms_kfdb_score_host(CmsKfdbBow{n1, id1, val1}, CmsKfdbBow{n2, id2, val2});
  return 0;
}

// ---- Covisibility (tests/covis_hostlib.py): the host build of csrc/cms_covis_core.h, the definition of record of cms_covis_*.  The calls mirror the
// C-ABI's on a handle of its own that also stands in for the store's rows (hm_covis_put: a slot's mp row and octaves); they return 0, -1
// (CMS_ERR_ARG), -3 (CMS_ERR_UNSUPPORTED) or -4 (CMS_ERR_OVERFLOW).
extern "C" int hm_covis_create(void** out, int max_keyframes, int max_features, int max_members) {
  HM_TRY(
    if (!out || max_keyframes < 1 || max_features < 1 || max_members < 1) throw std::runtime_error("hm_covis_create: bad argument");
    *out = new CmsCovisHostStore(max_keyframes, max_features, max_members);
    return 0;)
}
extern "C" void hm_covis_destroy(void* cv) { delete static_cast<CmsCovisHostStore*>(cv); }
extern "C" int hm_covis_put(void* cv, int slot, int n, const int* mp, const int* octave) { HM_TRY(return static_cast<CmsCovisHostStore*>(cv)->put(slot, n, mp, octave);) }
extern "C" int hm_covis_update_map_points(void* cv, int n, const int* slot, const int* feat, const int* mp) {
  HM_TRY(return static_cast<CmsCovisHostStore*>(cv)->update_map_points(n, slot, feat, mp);)
}
extern "C" int hm_covis_fetch_mp(void* cv, int slot, int* mp) {
  HM_TRY(
    CmsCovisHostStore* d = static_cast<CmsCovisHostStore*>(cv);
    if (!d->slot_ok(slot) || !d->slots[(size_t)slot].used) return -1;
    std::copy(d->slots[(size_t)slot].mp.begin(), d->slots[(size_t)slot].mp.end(), mp);
    return 0;)
}
extern "C" int hm_covis_build(void* cv, int n_members, const int* member_slots) { HM_TRY(return static_cast<CmsCovisHostStore*>(cv)->build(n_members, member_slots);) }
extern "C" int hm_covis_votes(void* cv, int njobs, const int* id_off, const int* ids, int* votes) {
  HM_TRY(return static_cast<CmsCovisHostStore*>(cv)->index.votes(njobs, id_off, ids, votes);)
}
extern "C" int hm_covis_connections(void* cv, int njobs, const int* job_member, int th, int* weights, int* order, int* n_connected) {
  HM_TRY(return static_cast<CmsCovisHostStore*>(cv)->index.connections(njobs, job_member, th, weights, order, n_connected);)
}
extern "C" int hm_covis_culling(void* cv, int n_chains, const int* chain_off, const int* job_member, const uint8_t* erasable, int th_obs, int* n_mps, int* n_redundant,
                                uint8_t* redundant) {
  HM_TRY(return static_cast<CmsCovisHostStore*>(cv)->index.culling(n_chains, chain_off, job_member, erasable, th_obs, n_mps, n_redundant, redundant);)
}
extern "C" int hm_covis_local_points(void* cv, int njobs, const int* kf_off, const int* kf_members, int cap, int* ids_out, int* n_out) {
  HM_TRY(return static_cast<CmsCovisHostStore*>(cv)->index.local_points(njobs, kf_off, kf_members, cap, ids_out, n_out);)
}

// ---- Map points (tests/mappoint_hostlib.py): the host build of csrc/cms_mappoint_core.h, the definition of record of cms_mpstore_*.  One handle stands
// in for the store (hm_mpstore_put: a slot's mp row, octaves, descriptors and camera centre), the index (hm_mpstore_build) and the table; the
// level scale factors come with the create call.  0, -1 (CMS_ERR_ARG: nothing was written) or -3 (CMS_ERR_UNSUPPORTED).
extern "C" int hm_mpstore_create(void** out, int max_keyframes, int max_features, int max_members, int max_points, int nlevels, const float* scale_factors) {
  HM_TRY(
    if (!out || max_keyframes < 1 || max_features < 1 || max_members < 1 || max_points < 1 || nlevels < 1 || nlevels > 16 || !scale_factors)
      throw std::runtime_error("hm_mpstore_create: bad argument");
    *out = new CmsMpHostStore(max_keyframes, max_features, max_members, max_points, nlevels, scale_factors);
    return 0;)
}
extern "C" void hm_mpstore_destroy(void* mp) { delete static_cast<CmsMpHostStore*>(mp); }
extern "C" int hm_mpstore_put(void* mp, int slot, int n, const int* ids, const int* octave, const uint8_t* desc, const float* Ow) {
  HM_TRY(return static_cast<CmsMpHostStore*>(mp)->put(slot, n, ids, octave, desc, Ow);)
}
extern "C" int hm_mpstore_update_poses(void* mp, int n, const int* slots, const float* Ow) { HM_TRY(return static_cast<CmsMpHostStore*>(mp)->update_poses(n, slots, Ow);) }
extern "C" int hm_mpstore_update_map_points(void* mp, int n, const int* slot, const int* feat, const int* ids) {
  HM_TRY(return static_cast<CmsMpHostStore*>(mp)->cv.update_map_points(n, slot, feat, ids);)
}
extern "C" int hm_mpstore_build(void* mp, int n_members, const int* member_slots) { HM_TRY(return static_cast<CmsMpHostStore*>(mp)->build(n_members, member_slots);) }
// the index's observations of an id in member order: up to cap (member, feature, octave) triples into out, their number into n_out
extern "C" int hm_mpstore_observations(void* mp, int id, int cap, int* out, int* n_out) {
  HM_TRY(
    const CmsCovisHost& ix = static_cast<CmsMpHostStore*>(mp)->cv.index;
    const int u = ix.find(id);
    *n_out = u < 0 ? 0 : ix.seg[(size_t)u + 1] - ix.seg[(size_t)u];
    for (int k = 0; k < *n_out && k < cap; ++k) {
      const CmsCovisHost::Obs& o = ix.obs[(size_t)ix.seg[(size_t)u] + (size_t)k];
      out[3 * k] = o.member; out[3 * k + 1] = o.feat; out[3 * k + 2] = o.octave;
    }
    return 0;)
}
extern "C" int hm_mpstore_set(void* mp, int n, const int* ids, const float* pos, const int* ref_slot) { HM_TRY(return static_cast<CmsMpHostStore*>(mp)->set(n, ids, pos, ref_slot);) }
extern "C" int hm_mpstore_erase(void* mp, int n, const int* ids) { HM_TRY(return static_cast<CmsMpHostStore*>(mp)->erase(n, ids);) }
extern "C" int hm_mpstore_refresh(void* mp, int n, const int* ids, int what, uint8_t* status) { HM_TRY(return static_cast<CmsMpHostStore*>(mp)->refresh(n, ids, what, status);) }
extern "C" int hm_mpstore_fetch(void* mp, int n, const int* ids, float* pos, float* normal, float* min_dist, float* max_dist, uint8_t* desc, int* best_member,
                                int* best_feature) {
  HM_TRY(return static_cast<CmsMpHostStore*>(mp)->fetch(n, ids, pos, normal, min_dist, max_dist, desc, best_member, best_feature);)
}

// ---- Map-point statistics (tests/mpstats_hostlib.py): the host build of csrc/cms_mpstats_core.h on the same handle, the definition of record of
// cms_mpstore_set_stats / add_stats / fetch_stats / count / culling, cms_covis_tracked_map_points and cms_kfstore_scene_median_depth.  0 or -1
// (CMS_ERR_ARG: nothing was written).
static bool hm_mpstats_off_ok(int njobs, const int* off) {
  if (njobs < 0 || (njobs > 0 && (!off || off[0] != 0))) return false;
  for (int j = 0; j < njobs; ++j) if (off[j + 1] < off[j]) return false;
  return true;
}
// has hm_mpstore_build succeeded yet?  (the device entries refuse a query without an index)
static bool hm_mpstats_built(const CmsMpHostStore& s) { return !s.cv.index.seg.empty(); }
// the full pose of slots (hm_mpstore_put leaves Rcw = I, tcw = -Ow; hm_mpstore_update_poses moves only Ow)
extern "C" int hm_mpstats_update_poses(void* mp, int n, const int* slots, const float* Rcw, const float* tcw, const float* Ow) {
  HM_TRY(
    CmsMpHostStore& s = *static_cast<CmsMpHostStore*>(mp);
    if (s.update_poses(n, slots, Ow)) return -1;
    for (int i = 0; i < n; ++i) { memcpy(&s.Rcw[(size_t)slots[i] * 9], Rcw + 9 * (size_t)i, 36); memcpy(&s.tcw[(size_t)slots[i] * 3], tcw + 3 * (size_t)i, 12); }
    return 0;)
}
extern "C" int hm_mpstats_set_stats(void* mp, int n, const int* ids, const int* first_kf, const int* visible, const int* found) {
  HM_TRY(
    CmsMpHostStore& s = *static_cast<CmsMpHostStore*>(mp);
    if (n < 0 || (n > 0 && !ids) || !s.ids_ok(n, ids)) return -1;
    for (int i = 0; i < n; ++i) {
      if (!(s.rows[(size_t)ids[i]].state & 1)) return -1;
      if ((first_kf && first_kf[i] < -1) || (visible && visible[i] < 1) || (found && found[i] < 0)) return -1;
    }
    for (int i = 0; i < n; ++i) {
      CmsMpHostStore::Row& r = s.rows[(size_t)ids[i]];
      if (first_kf) r.first_kf = first_kf[i];
      if (visible) r.visible = visible[i];
      if (found) r.found = found[i];
    }
    return 0;)
}
extern "C" int hm_mpstats_add_stats(void* mp, int n, const int* ids, const int* d_visible, const int* d_found) {
  HM_TRY(
    CmsMpHostStore& s = *static_cast<CmsMpHostStore*>(mp);
    if (n < 0 || (n > 0 && !ids) || !s.ids_ok(n, ids)) return -1;
    for (int i = 0; i < n; ++i)
      if (!(s.rows[(size_t)ids[i]].state & 1) || (d_visible && d_visible[i] < 0) || (d_found && d_found[i] < 0)) return -1;
    for (int i = 0; i < n; ++i) {
      CmsMpHostStore::Row& r = s.rows[(size_t)ids[i]];
      if (d_visible) r.visible += d_visible[i];
      if (d_found) r.found += d_found[i];
    }
    return 0;)
}
extern "C" int hm_mpstats_fetch_stats(void* mp, int n, const int* ids, int* visible, int* found, int* first_kf) {
  HM_TRY(
    const CmsMpHostStore& s = *static_cast<CmsMpHostStore*>(mp);
    if (n < 0 || (n > 0 && !ids)) return -1;
    for (int i = 0; i < n; ++i) if (!s.id_ok(ids[i])) return -1;
    for (int i = 0; i < n; ++i) {
      const CmsMpHostStore::Row& r = s.rows[(size_t)ids[i]];
      if (visible) visible[i] = r.visible;
      if (found) found[i] = r.found;
      if (first_kf) first_kf[i] = r.first_kf;
    }
    return 0;)
}
extern "C" int hm_mpstats_count(void* mp, int which, int njobs, const int* off, const int* ids, const uint8_t* flag, int count_if) {
  HM_TRY(
    CmsMpHostStore& s = *static_cast<CmsMpHostStore*>(mp);
    if ((which != CMS_MP_VISIBLE && which != CMS_MP_FOUND) || !hm_mpstats_off_ok(njobs, off)) return -1;
    const int T = njobs > 0 ? off[njobs] : 0;
    if (T > 0 && !ids) return -1;
    auto counted = [&](int i) { return ids[i] >= 0 && (!flag || (flag[i] != 0) == (count_if != 0)); };
    for (int i = 0; i < T; ++i) {
      if (ids[i] < -1 || ids[i] >= (int)s.rows.size()) return -1;
      if (counted(i) && !(s.rows[(size_t)ids[i]].state & 1)) return -1;
    }
    for (int i = 0; i < T; ++i)
      if (counted(i)) ++(which == CMS_MP_VISIBLE ? s.rows[(size_t)ids[i]].visible : s.rows[(size_t)ids[i]].found);
    return 0;)
}
extern "C" int hm_mpstats_culling(void* mp, int njobs, const int* off, const int* ids, const int* current_kf, int th_obs, int apply, uint8_t* verdict) {
  HM_TRY(
    CmsMpHostStore& s = *static_cast<CmsMpHostStore*>(mp);
    if (th_obs < 0 || !hm_mpstats_off_ok(njobs, off) || !hm_mpstats_built(s)) return -1;
    const int n = njobs > 0 ? off[njobs] : 0;
    if ((njobs > 0 && !current_kf) || (n > 0 && (!ids || !verdict)) || !s.ids_ok(n, ids)) return -1;
    const CmsCovisHost& ix = s.cv.index;
    for (int j = 0; j < njobs; ++j)
      for (int i = off[j]; i < off[j + 1]; ++i) {
        const CmsMpHostStore::Row& r = s.rows[(size_t)ids[i]];
        const int u = ix.find(ids[i]);
        const int n_obs = u < 0 ? 0 : ix.seg[(size_t)u + 1] - ix.seg[(size_t)u];
        verdict[i] = (uint8_t)((r.state & 1) ? cms_mpstats_verdict(r.found, r.visible, r.first_kf, n_obs, current_kf[j], th_obs) : CMS_MP_ALREADY_BAD);
      }
    if (!apply) return 0;
    for (int i = 0; i < n; ++i) {      // MapPoint::SetBadFlag (MapPoint.cpp:115-136)
      if (verdict[i] != CMS_MP_BAD_RATIO && verdict[i] != CMS_MP_BAD_FEW_OBS) continue;
      const int u = ix.find(ids[i]);
      if (u >= 0)
        for (int e = ix.seg[(size_t)u]; e < ix.seg[(size_t)u + 1]; ++e) {
          std::vector<int>& row = s.cv.slots[(size_t)s.member_slot[(size_t)ix.obs[(size_t)e].member]].mp;
          const size_t f = (size_t)ix.obs[(size_t)e].feat;
          if (f < row.size() && row[f] == ids[i]) row[f] = -1;      // (an entry changed since the build is left alone)
        }
      s.rows[(size_t)ids[i]] = CmsMpHostStore::Row();
    }
    return 0;)
}
extern "C" int hm_mpstats_tracked_map_points(void* mp, int njobs, const int* job_member, const int* min_obs, int* count) {
  HM_TRY(
    const CmsMpHostStore& s = *static_cast<CmsMpHostStore*>(mp);
    const CmsCovisHost& ix = s.cv.index;
    if (njobs < 0 || (njobs > 0 && (!job_member || !min_obs || !count)) || !hm_mpstats_built(s)) return -1;
    for (int j = 0; j < njobs; ++j) if (job_member[j] < 0 || job_member[j] >= ix.n_members) return -1;
    for (int j = 0; j < njobs; ++j) {
      int c = 0;
      for (int id : ix.mp[(size_t)job_member[j]]) {
        if (id < 0) continue;
        const int u = ix.find(id);      // (an id of the snapshot is in the index; the test keeps the function on its own feet)
        const int n_obs = u < 0 ? 0 : ix.seg[(size_t)u + 1] - ix.seg[(size_t)u];
        if (min_obs[j] <= 0 || n_obs >= min_obs[j]) ++c;
      }
      count[j] = c;
    }
    return 0;)
}
extern "C" int hm_mpstats_scene_median_depth(void* mp, int n, const int* slots, int q, int store, float* depth, int* n_depths) {
  HM_TRY(
    CmsMpHostStore& s = *static_cast<CmsMpHostStore*>(mp);
    if (n < 0 || q < 1 || (n > 0 && (!slots || !depth || !n_depths))) return -1;
    std::vector<uint8_t> seen(s.cv.slots.size(), 0);
    for (int i = 0; i < n; ++i) {
      if (!s.cv.slot_ok(slots[i]) || !s.cv.slots[(size_t)slots[i]].used || seen[(size_t)slots[i]]) return -1;
      seen[(size_t)slots[i]] = 1;
    }
    for (int i = 0; i < n; ++i) {
      const size_t sl = (size_t)slots[i];
      std::vector<uint32_t> key;
      for (int id : s.cv.slots[sl].mp)
        if (s.id_ok(id) && (s.rows[(size_t)id].state & 1)) key.push_back(cms_mpstats_depth_key(cms_mpstats_depth(&s.Rcw[sl * 9], &s.tcw[sl * 3], s.rows[(size_t)id].pos)));
      n_depths[i] = (int)key.size();
      if (key.empty()) { depth[i] = -1.0f; continue; }
      // the smallest key v with #(key <= v) > idx, by bisection on the 32 bits: the rule as cms_mpstats_core.h words it
      const int idx = cms_mpstats_depth_index((int)key.size(), q);
      uint32_t lo = 0u, hi = 0xFFFFFFFFu;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        int c = 0;
        for (uint32_t k : key) c += k <= mid;
        if (c > idx) hi = mid; else lo = mid + 1u;
      }
      depth[i] = cms_mpstats_depth_from_key(lo);
      if (store) s.median[sl] = depth[i];
    }
    return 0;)
}
// a slot's mp row as the stand-in of the store holds it now (n entries: what hm_mpstore_put gave)
extern "C" int hm_mpstats_fetch_mp(void* mp, int slot, int cap, int* out, int* n_out) {
  HM_TRY(
    const CmsMpHostStore& s = *static_cast<CmsMpHostStore*>(mp);
    if (!s.cv.slot_ok(slot) || !s.cv.slots[(size_t)slot].used) return -1;
    const std::vector<int>& row = s.cv.slots[(size_t)slot].mp;
    *n_out = (int)row.size();
    for (size_t f = 0; f < row.size() && f < (size_t)cap; ++f) out[f] = row[f];
    return 0;)
}
extern "C" int hm_mpstats_fetch_median(void* mp, int slot, float* median) {
  HM_TRY(
    const CmsMpHostStore& s = *static_cast<CmsMpHostStore*>(mp);
    if (!s.cv.slot_ok(slot)) return -1;
    *median = s.median[(size_t)slot];
    return 0;)
}

// ---- Local BA window (tests/ba_window_hostlib.py): the host build of csrc/cms_ba_window_core.h, the definition of record of cms_covis_local_ba_windows.
// One handle holds what the walk reads: the index over n_members rows (n_feat[m] features each; mp, octave, key-point x / y and the rays' z
// concatenated), the members' Rcw (9 floats) and tcw (3), the table's rows that hold a position (n_pos ids with 3 floats each, ids below max_points),
// mvInvLevelSigma2, and the camera of hm_set_camera (face width, cos_fov).  hm_ba_window_run assembles njobs windows (job j: the members
// local_members[local_off[j], local_off[j + 1]) and first_member[j]) into row j of every output.  0, -1 (CMS_ERR_ARG: nothing was written, hm_last_error
// says why) or -4 (CMS_ERR_OVERFLOW).
struct HmBaWindow { CmsCovisHost ix; CmsBaWindowHostData D; };
extern "C" int hm_ba_window_create(void** out, int n_members, const int* n_feat, const int* mp, const int* octave, const float* kp_x, const float* kp_y, const float* ray_z,
                                   const float* Rcw, const float* tcw, int max_points, int n_pos, const int* pos_ids, const float* pos, int nlevels, const float* inv_sigma2) {
  HM_TRY(
    if (!out || n_members < 0 || max_points < 1 || n_pos < 0 || nlevels < 1 || nlevels > 16 || !inv_sigma2) throw std::runtime_error("hm_ba_window_create: bad argument");
    std::unique_ptr<HmBaWindow> w(new HmBaWindow());
    std::vector<const int*> rows((size_t)n_members), octs((size_t)n_members);
    CmsBaWindowHostData& D = w->D;
    D.kx.resize((size_t)n_members); D.ky.resize((size_t)n_members); D.ray_z.resize((size_t)n_members);
    size_t at = 0;
    for (int m = 0; m < n_members; ++m) {
      const size_t n = (size_t)n_feat[m];
      rows[(size_t)m] = mp + at; octs[(size_t)m] = octave + at;
      for (size_t f = 0; f < n; ++f) if (octave[at + f] < 0 || octave[at + f] >= nlevels) throw std::runtime_error("hm_ba_window_create: an octave outside the pyramid");
      D.kx[(size_t)m].assign(kp_x + at, kp_x + at + n); D.ky[(size_t)m].assign(kp_y + at, kp_y + at + n); D.ray_z[(size_t)m].assign(ray_z + at, ray_z + at + n);
      at += n;
    }
    if (w->ix.build(n_members, n_feat, rows.data(), octs.data())) throw std::runtime_error("hm_ba_window_create: the index refuses the rows");
    D.Rcw.assign(Rcw, Rcw + 9 * (size_t)n_members); D.tcw.assign(tcw, tcw + 3 * (size_t)n_members);
    D.has_pos.assign((size_t)max_points, 0); D.pos.assign(3 * (size_t)max_points, 0.0f);
    for (int i = 0; i < n_pos; ++i) {
      if (pos_ids[i] < 0 || pos_ids[i] >= max_points) throw std::runtime_error("hm_ba_window_create: an id outside the table");
      D.has_pos[(size_t)pos_ids[i]] = 1;
      std::memcpy(&D.pos[3 * (size_t)pos_ids[i]], pos + 3 * (size_t)i, 12);
    }
    for (int l = 0; l < 16; ++l) D.inv_sigma2[l] = l < nlevels ? inv_sigma2[l] : 0.0f;
    const CamModelGeneral* cam = CamModelGeneral::GetCamera();
    D.F = cam->GetCubeFaceWidth(); D.cos_fov = cam->GetCosFovTh();
    *out = w.release();
    return 0;)
}
extern "C" void hm_ba_window_destroy(void* w) { delete static_cast<HmBaWindow*>(w); }
extern "C" int hm_ba_window_run(void* handle, int njobs, const int* local_off, const int* local_members, const int* first_member, int cap_kf, int cap_points, int cap_edges,
                                int* counts, int* kf_member, int* point_id, double* poses, uint8_t* fixed, double* points, int* e_pose, int* e_point, double* e_obs,
                                double* e_invsig2, int8_t* e_face, int* e_feat) {
  HM_TRY(
    const HmBaWindow* w = static_cast<const HmBaWindow*>(handle);
    if (!w || njobs < 0 || (njobs > 0 && (!local_off || !first_member))) throw std::runtime_error("hm_ba_window_run: bad argument");
    std::vector<CmsBaWindowHostJob> jobs((size_t)njobs);
    for (int j = 0; j < njobs; ++j) jobs[(size_t)j] = CmsBaWindowHostJob{local_off[j + 1] - local_off[j], local_members + local_off[j], first_member[j]};
    const CmsBaWindowHostOut o = {cap_kf, cap_points, cap_edges, reinterpret_cast<CmsBaWindowCounts*>(counts), kf_member, point_id, poses, fixed, points,
                                  e_pose, e_point, e_obs, e_invsig2, e_face, e_feat};
    std::string why;
    const int rc = cms_ba_window_host(w->ix, w->D, njobs, jobs.data(), o, &why);
    if (rc == -1) g_err = "hm_ba_window_run: " + why;
    return rc;)
}

// CubemapSLAM::MapPointStore::LocalBAWindow of the mirror through the named engine (0 = device, 1 = host core): n_kf key frames (features concatenated: mp,
// octave, key-point x / y, rays 3 floats each; Tcw 16 floats and mnId each) are the members, n_pts points (id, position, reference key frame as an
// index) are set, the window of local_kf[0, n_local) is assembled into the arrays (caps as given; -4 when it does not fit), key frames as member
// indices.  run_ba: Optimizer::LocalBundleAdjustment(mps, &window) behind it -- poses and points are then the optimised ones, n_erase the
// observations to erase, and the members' Tcw after the write-back come back in Tcw_out (16 floats each).
extern "C" int hm_ba_window_mirror(int engine, int n_kf, const int* n_feat, const int* mp, const int* octave, const float* kp_x, const float* kp_y, const float* rays,
                                   const float* Tcw16, const int* mn_id, int max_points, int n_pts, const int* ids, const float* pos, const int* ref_kf, int n_local,
                                   const int* local_kf, int run_ba, int cap_kf, int cap_points, int cap_edges, int* counts, int* kf_member, int* point_id, double* poses,
                                   uint8_t* fixed, double* points, int* e_pose, int* e_point, double* e_obs, double* e_invsig2, int8_t* e_face, int* e_feat, int* n_erase,
                                   float* Tcw_out) {
  HM_TRY(
    std::vector<KeyFrameView> kfs((size_t)n_kf);
    std::vector<KeyFrameView*> members;
    int max_feat = 1;
    size_t at = 0;
    for (int k = 0; k < n_kf; ++k) {
      KeyFrameView& v = kfs[(size_t)k];
      const int n = n_feat[k];
      max_feat = std::max(max_feat, n);
      v.mnId = mn_id[k];
      v.mDescriptors = cv::Mat::zeros(std::max(n, 1), 32, cv::CV_8U);
      v.mvKeys.resize((size_t)n); v.mvKeyRays.resize((size_t)n); v.mvpMapPoints.resize((size_t)n);
      for (int f = 0; f < n; ++f) {
        const size_t i = at + (size_t)f;
        v.mvKeys[(size_t)f].pt.x = kp_x[i]; v.mvKeys[(size_t)f].pt.y = kp_y[i]; v.mvKeys[(size_t)f].octave = octave[i];
        for (int c = 0; c < 3; ++c) v.mvKeyRays[(size_t)f].v[c] = rays[3 * i + (size_t)c];
        v.mvpMapPoints[(size_t)f] = mp[i];
      }
      at += (size_t)n;
      v.Tcw = cv::Mat::zeros(4, 4, cv::CV_32F);
      for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) v.Tcw.at<float>(r, c) = Tcw16[16 * (size_t)k + 4 * (size_t)r + (size_t)c];
      members.push_back(&v);
    }
    MapPointStore mps(engine ? MapPointStore::HOST_CORE : MapPointStore::DEVICE, n_kf + 1, max_feat, max_points);
    mps.Build(members);
    std::vector<MapPointStore::MapPointView> pts((size_t)n_pts);
    for (int i = 0; i < n_pts; ++i) {
      pts[(size_t)i].id = ids[i];
      std::memcpy(pts[(size_t)i].pos, pos + 3 * (size_t)i, 12);
      pts[(size_t)i].pRefKF = &kfs[(size_t)ref_kf[i]];
    }
    mps.SetMapPoints(pts);
    std::vector<KeyFrameView*> local;
    for (int i = 0; i < n_local; ++i) local.push_back(&kfs[(size_t)local_kf[i]]);
    MapPointStore::BAWindow w = mps.LocalBAWindow(local);
    *n_erase = 0;
    if (run_ba) {
      Optimizer::LocalBundleAdjustment(mps, &w, nullptr);
      *n_erase = (int)w.toErase.size();
      for (int k = 0; k < n_kf; ++k)
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) Tcw_out[16 * (size_t)k + 4 * (size_t)r + (size_t)c] = kfs[(size_t)k].Tcw.at<float>(r, c);
    }
    const int K = (int)w.keyframes.size(), P = (int)w.point_id.size(), E = (int)w.e_pose.size();
    counts[0] = K; counts[1] = w.nLocal; counts[2] = P; counts[3] = E;
    if (K > cap_kf || P > cap_points || E > cap_edges) return -4;
    for (int k = 0; k < K; ++k) kf_member[k] = (int)(w.keyframes[(size_t)k] - kfs.data());
    for (int p = 0; p < P; ++p) point_id[p] = (int)w.point_id[(size_t)p];
    std::copy(w.poses.begin(), w.poses.end(), poses); std::copy(w.fixed.begin(), w.fixed.end(), fixed); std::copy(w.points.begin(), w.points.end(), points);
    std::copy(w.e_pose.begin(), w.e_pose.end(), e_pose); std::copy(w.e_point.begin(), w.e_point.end(), e_point); std::copy(w.e_obs.begin(), w.e_obs.end(), e_obs);
    std::copy(w.e_invsig2.begin(), w.e_invsig2.end(), e_invsig2); std::copy(w.e_face.begin(), w.e_face.end(), e_face); std::copy(w.e_feat.begin(), w.e_feat.end(), e_feat);
    return 0;)
}

// the key-frame views of the two MapPointStore mirrors below: n_kf key frames of n_feat[k] features (mp, octave and descriptor rows concatenated -- desc
// may be NULL: zeros --, Tcw 16 floats each); returns the longest row
static int hm_mirror_views(int n_kf, const int* n_feat, const int* mp, const int* octave, const uint8_t* desc, const float* Tcw16, std::vector<KeyFrameView>& kfs,
                           std::vector<KeyFrameView*>& members) {
  kfs.assign((size_t)n_kf, KeyFrameView());
  members.clear();
  int max_feat = 1;
  size_t at = 0;
  for (int k = 0; k < n_kf; ++k) {
    KeyFrameView& v = kfs[(size_t)k];
    const int n = n_feat[k];
    max_feat = std::max(max_feat, n);
    v.mnId = k + 1;
    v.mDescriptors = cv::Mat::zeros(std::max(n, 1), 32, cv::CV_8U);
    v.mvKeys.resize((size_t)n);
    cv::Vec3f ray;
    ray.v[0] = 0.f; ray.v[1] = 0.f; ray.v[2] = 1.f;
    v.mvKeyRays.assign((size_t)n, ray);
    v.mvpMapPoints.resize((size_t)n);
    for (int f = 0; f < n; ++f) {
      v.mvKeys[(size_t)f].pt.x = 10.f + (float)(f % 100); v.mvKeys[(size_t)f].pt.y = 10.f + (float)(f / 100); v.mvKeys[(size_t)f].octave = octave[at + (size_t)f];
      v.mvpMapPoints[(size_t)f] = mp[at + (size_t)f];
      if (desc) std::memcpy(v.mDescriptors.ptr<uint8_t>(f), desc + 32 * (at + (size_t)f), 32);
    }
    at += (size_t)n;
    v.Tcw = cv::Mat::zeros(4, 4, cv::CV_32F);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) v.Tcw.at<float>(r, c) = Tcw16[16 * (size_t)k + 4 * (size_t)r + (size_t)c];
    members.push_back(&v);
  }
  return max_feat;
}

// CubemapSLAM::MapPointStore of the mirror through the named engine (0 = device, 1 = host core): n_kf key frames of n_feat[k] features (mp, octave and
// descriptor rows concatenated, Tcw 16 floats each) are the members; n_pts points (id, position, reference key frame as an index) are set, refreshed
// with `what` and fetched: status, normal, distances, descriptor, the best observation's key frame (index or -1) and feature per point.
extern "C" int hm_mpstore_mirror(int engine, int n_kf, const int* n_feat, const int* mp, const int* octave, const uint8_t* desc, const float* Tcw16, int max_points, int n_pts,
                                 const int* ids, const float* pos, const int* ref_kf, int what, uint8_t* status, float* normal, float* min_dist, float* max_dist,
                                 uint8_t* out_desc, int* best_kf, int* best_idx) {
  HM_TRY(
    std::vector<KeyFrameView> kfs;
    std::vector<KeyFrameView*> members;
    const int max_feat = hm_mirror_views(n_kf, n_feat, mp, octave, desc, Tcw16, kfs, members);
    MapPointStore mps(engine ? MapPointStore::HOST_CORE : MapPointStore::DEVICE, n_kf + 1, max_feat, max_points);
    mps.Build(members);
    std::vector<MapPointStore::MapPointView> pts((size_t)n_pts);
    std::vector<long> lids((size_t)n_pts);
    for (int i = 0; i < n_pts; ++i) {
      pts[(size_t)i].id = ids[i]; lids[(size_t)i] = ids[i];
      std::memcpy(pts[(size_t)i].pos, pos + 3 * (size_t)i, 12);
      pts[(size_t)i].pRefKF = &kfs[(size_t)ref_kf[i]];
    }
    mps.SetMapPoints(pts);
    const std::vector<unsigned char> st = mps.Refresh(lids, what);
    const std::vector<MapPointStore::Row> rows = mps.Fetch(lids);
    for (int i = 0; i < n_pts; ++i) {
      const MapPointStore::Row& r = rows[(size_t)i];
      status[i] = st[(size_t)i];
      std::memcpy(normal + 3 * (size_t)i, r.normal, 12); min_dist[i] = r.minDistance; max_dist[i] = r.maxDistance;
      std::memcpy(out_desc + 32 * (size_t)i, r.descriptor, 32);
      best_kf[i] = r.pBestKF ? (int)(r.pBestKF - kfs.data()) : -1; best_idx[i] = r.bestIdx;
    }
    return 0;)
}

// The statistics methods of the mirror's MapPointStore through the named engine, one mapping step: Build over the key frames, SetMapPoints (every point
// refers to key frame 0), SetStatistics(first_kf), UpdateTrackStatistics per frame (frame f: the ids [frame_off[f], frame_off[f + 1]) with their
// in_view and outlier flags, used both as the local and as the frame's list), MapPointCulling of all points in id order with current_kf, a second
// Build over the views as the culling left them, then TrackedMapPoints(min_obs) and ComputeSceneMedianDepth(q) of every key frame.
// verdict / stats (first_kf, visible, found per point, after the culling) / n_left (the list's length) / mp_out (the views' rows) / tracked / depth
extern "C" int hm_mpstats_mirror(int engine, int n_kf, const int* n_feat, const int* mp, const int* octave, const float* Tcw16, int max_points, int n_pts, const int* ids,
                                 const float* pos, const int* first_kf, int n_frames, const int* frame_off, const int* frame_ids, const uint8_t* in_view,
                                 const uint8_t* outlier, int current_kf, int min_obs, int q, uint8_t* verdict, int* stats, int* n_left, int* mp_out, int* tracked,
                                 float* depth) {
  HM_TRY(
    std::vector<KeyFrameView> kfs;
    std::vector<KeyFrameView*> members;
    const int max_feat = hm_mirror_views(n_kf, n_feat, mp, octave, nullptr, Tcw16, kfs, members);
    MapPointStore mps(engine ? MapPointStore::HOST_CORE : MapPointStore::DEVICE, n_kf + 1, max_feat, max_points);
    mps.Build(members);
    std::vector<MapPointStore::MapPointView> pts((size_t)n_pts);
    std::vector<MapPointStore::MapPointStats> st((size_t)n_pts);
    std::list<long> recent;
    std::vector<long> lids((size_t)n_pts);
    for (int i = 0; i < n_pts; ++i) {
      pts[(size_t)i].id = ids[i]; lids[(size_t)i] = ids[i];
      std::memcpy(pts[(size_t)i].pos, pos + 3 * (size_t)i, 12);
      pts[(size_t)i].pRefKF = &kfs[0];
      st[(size_t)i] = MapPointStore::MapPointStats{ids[i], first_kf[i], -1, -1};
      recent.push_back(ids[i]);
    }
    mps.SetMapPoints(pts);
    mps.SetStatistics(st);
    for (int f = 0; f < n_frames; ++f) {
      const int a = frame_off[f], b = frame_off[f + 1];
      const std::vector<long> fid(frame_ids + a, frame_ids + b);
      mps.UpdateTrackStatistics(fid, std::vector<unsigned char>(in_view + a, in_view + b), fid, std::vector<unsigned char>(outlier + a, outlier + b));
    }
    const std::vector<unsigned char> v = mps.MapPointCulling(recent, current_kf);
    std::copy(v.begin(), v.end(), verdict);
    *n_left = (int)recent.size();
    const std::vector<MapPointStore::MapPointStats> after = mps.FetchStatistics(lids);
    for (int i = 0; i < n_pts; ++i) { stats[3 * i] = after[(size_t)i].nFirstKFid; stats[3 * i + 1] = after[(size_t)i].nVisible; stats[3 * i + 2] = after[(size_t)i].nFound; }
    size_t at = 0;
    for (int k = 0; k < n_kf; ++k) for (long id : kfs[(size_t)k].mvpMapPoints) mp_out[at++] = (int)id;
    mps.Build(members);
    for (int k = 0; k < n_kf; ++k) { tracked[k] = mps.TrackedMapPoints(&kfs[(size_t)k], min_obs); depth[k] = mps.ComputeSceneMedianDepth(&kfs[(size_t)k], q); }
    return 0;)
}

// CubemapSLAM::Covisibility of the mirror through the named engine (0 = device, 1 = host core): n_kf key frames of n_feat[k] features (mp and octave rows
// concatenated) are the members; then UpdateConnections for conn_kf[0, n_conn) (the ordered key frames of all, concatenated, into `ordered` with
// their weights; n_ordered[i] each), ONE KeyFrameCulling over cull_kf[0, n_cull) with not_erase (nMPs, nRedundantObservations, verdict),
// UpdateLocalKeyFrames for the frame's ids (the local key frames into local_kf, n_local, pKFmax as an index or -1) and UpdateLocalPoints over
// lp_kf[0, n_lp) (ids into lp_ids, cap lp_cap, n_lp_ids).
extern "C" int hm_covis_mirror(int engine, int n_kf, const int* n_feat, const int* mp, const int* octave, int n_conn, const int* conn_kf, int* ordered, int* ordered_w,
                               int* n_ordered, int n_cull, const int* cull_kf, const uint8_t* not_erase, int* cull_nmps, int* cull_nred, uint8_t* cull_red, int n_ids,
                               const int* ids, int* local_kf, int* n_local, int* kf_max, int n_lp, const int* lp_kf, int lp_cap, int* lp_ids, int* n_lp_ids) {
  HM_TRY(
    std::vector<KeyFrameView> kfs((size_t)n_kf);
    std::vector<KeyFrameView*> members;
    int max_feat = 1;
    size_t at = 0;
    for (int k = 0; k < n_kf; ++k) {
      KeyFrameView& v = kfs[(size_t)k];
      const int n = n_feat[k];
      max_feat = std::max(max_feat, n);
      v.mnId = k + 1;
      v.mDescriptors = cv::Mat::zeros(std::max(n, 1), 32, cv::CV_8U);
      v.mvKeys.resize((size_t)n);
      cv::Vec3f ray;
      ray.v[0] = 0.f; ray.v[1] = 0.f; ray.v[2] = 1.f;
      v.mvKeyRays.assign((size_t)n, ray);
      v.mvpMapPoints.resize((size_t)n);
      for (int f = 0; f < n; ++f) {
        v.mvKeys[(size_t)f].pt.x = 10.f + (float)(f % 100); v.mvKeys[(size_t)f].pt.y = 10.f + (float)(f / 100); v.mvKeys[(size_t)f].octave = octave[at + (size_t)f];
        v.mvpMapPoints[(size_t)f] = mp[at + (size_t)f];
      }
      at += (size_t)n;
      v.Tcw = cv::Mat::zeros(4, 4, cv::CV_32F);
      for (int r = 0; r < 4; ++r) v.Tcw.at<float>(r, r) = 1.f;
      members.push_back(&v);
    }
    auto index_of = [&](KeyFrameView* k) { return (int)(k - kfs.data()); };
    Covisibility cvs(engine ? Covisibility::HOST_CORE : Covisibility::DEVICE, n_kf + 1, max_feat);
    cvs.Build(members);
    size_t o = 0;
    for (int i = 0; i < n_conn; ++i) {
      const Covisibility::Connections c = cvs.UpdateConnections(&kfs[(size_t)conn_kf[i]]);
      n_ordered[i] = (int)c.ordered.size();
      for (size_t q = 0; q < c.ordered.size(); ++q, ++o) { ordered[o] = index_of(c.ordered[q]); ordered_w[o] = c.orderedWeights[q]; }
    }
    std::vector<KeyFrameView*> cand;
    std::vector<bool> ne;
    for (int i = 0; i < n_cull; ++i) { cand.push_back(&kfs[(size_t)cull_kf[i]]); ne.push_back(not_erase[i] != 0); }
    const std::vector<Covisibility::Culled> cu = cvs.KeyFrameCulling(cand, ne);
    for (size_t i = 0; i < cu.size(); ++i) { cull_nmps[i] = cu[i].nMPs; cull_nred[i] = cu[i].nRedundantObservations; cull_red[i] = cu[i].redundant ? 1 : 0; }
    KeyFrameView* best = nullptr;
    const std::vector<KeyFrameView*> local = cvs.UpdateLocalKeyFrames(std::vector<long>(ids, ids + n_ids), &best);
    *n_local = (int)local.size();
    for (size_t i = 0; i < local.size(); ++i) local_kf[i] = index_of(local[i]);
    *kf_max = best ? index_of(best) : -1;
    std::vector<KeyFrameView*> lp;
    for (int i = 0; i < n_lp; ++i) lp.push_back(&kfs[(size_t)lp_kf[i]]);
    const std::vector<long> pts = cvs.UpdateLocalPoints(lp);
    *n_lp_ids = (int)pts.size();
    for (size_t i = 0; i < pts.size() && (int)i < lp_cap; ++i) lp_ids[i] = (int)pts[i];
    return 0;)
}

// ORB_SLAM2::KeyFrameDatabase of the mirror through the named engine (0 = device, 1 = host core): n_kf key frames of n_feat descriptors each enter in
// order (their BoW from the vocabulary's host core, levelsup 1), covis holds n_kf x 10 key-frame indices (-1 padded); then one
// DetectRelocalizationCandidates for a frame of nq descriptors and one DetectLoopCandidates for key frame loop_query.  The candidates come back as
// key-frame indices (arrays of n_kf).
extern "C" int hm_kfdb_mirror(void* voc, int engine, int n_kf, int n_feat, const uint8_t* descs, const int* covis, int nq, const uint8_t* qdesc, int loop_query,
                              float min_score, int n_conn, const int* conn, int* reloc, int* n_reloc, int* loop, int* n_loop) {
  HM_TRY(
    ORBVocabulary* v = static_cast<ORBVocabulary*>(voc);
    v->engine = ORBVocabulary::HOST_CORE;
    std::vector<KeyFrameView> kfs((size_t)n_kf);
    KeyFrameDatabase db(*v, n_kf + 1, 2048);
    db.engine = engine ? KeyFrameDatabase::HOST_CORE : KeyFrameDatabase::DEVICE;
    auto index_of = [&](KeyFrameView* k) { return (int)(k - kfs.data()); };
    for (int i = 0; i < n_kf; ++i) {
      KeyFrameView& k = kfs[(size_t)i];
      k.mnId = i;
      k.mDescriptors = cv::Mat(n_feat, 32, cv::CV_8U, const_cast<uint8_t*>(descs) + 32 * (size_t)i * n_feat, 32);
      k.mvKeys.resize((size_t)n_feat);
      for (int f = 0; f < n_feat; ++f) { k.mvKeys[(size_t)f].pt.x = 10.f + (float)(f % 100); k.mvKeys[(size_t)f].pt.y = 10.f + (float)(f / 100); }
      cv::Vec3f ray;
      ray.v[0] = 0.f; ray.v[1] = 0.f; ray.v[2] = 1.f;
      k.mvKeyRays.assign((size_t)n_feat, ray);
      k.mvpMapPoints.assign((size_t)n_feat, -1);
      k.Tcw = cv::Mat::zeros(4, 4, cv::CV_32F);
      for (int r = 0; r < 4; ++r) k.Tcw.at<float>(r, r) = 1.f;
      v->transform(std::vector<cv::Mat>(), k.mBowVec, k.mFeatVec, 1);
      std::vector<cv::Mat> rows((size_t)n_feat);
      for (int f = 0; f < n_feat; ++f) rows[(size_t)f] = k.mDescriptors.row(f);
      v->transform(rows, k.mBowVec, k.mFeatVec, 1);
      db.add(&k);
    }
    for (int i = 0; i < n_kf; ++i) {
      std::vector<KeyFrameView*> best;
      for (int c = 0; c < 10; ++c) if (covis[i * 10 + c] >= 0) best.push_back(&kfs[(size_t)covis[i * 10 + c]]);
      db.SetBestCovisibilityKeyFrames(&kfs[(size_t)i], best);
    }
    FrameView F;
    std::vector<cv::Mat> rows((size_t)nq);
    cv::Mat Q(std::max(nq, 1), 32, cv::CV_8U, const_cast<uint8_t*>(qdesc), 32);
    for (int f = 0; f < nq; ++f) rows[(size_t)f] = Q.row(f);
    v->transform(rows, F.mBowVec, F.mFeatVec, 1);
    const std::vector<KeyFrameView*> r = db.DetectRelocalizationCandidates(&F);
    *n_reloc = (int)r.size();
    for (size_t i = 0; i < r.size(); ++i) reloc[i] = index_of(r[i]);
    std::vector<KeyFrameView*> connected;
    for (int i = 0; i < n_conn; ++i) connected.push_back(&kfs[(size_t)conn[i]]);
    const std::vector<KeyFrameView*> l = db.DetectLoopCandidates(&kfs[(size_t)loop_query], min_score, connected);
    *n_loop = (int)l.size();
    for (size_t i = 0; i < l.size(); ++i) loop[i] = index_of(l[i]);
    return 0;)
}

// Optimizer::OptimizeEssentialGraph of cubemap_hot_path.h over flat arrays.  Key frames: mnId, bad, Tcw (12 floats, in/out), parent, and three lists
// in CSR form (children, loop edges, covisibles with weights by descending weight).  Map points: bad, pos (in/out), reference key frame,
// mnCorrectedByKF, mnCorrectedReference.  The pose maps as (key frame, 8 doubles) rows, LoopConnections in CSR form.  Out: the graph
// CollectEssentialGraph made (N, E, vertex_kf, edges, fixed) with capacities cap_v / cap_e
extern "C" int hm_ess_graph_mirror(int engine, int nkf, const int* mnId, const uint8_t* bad, float* Tcw, const int* parent, const int* child_off, const int* child,
                                   const int* loop_off, const int* loop, const int* cov_off, const int* cov, const int* cov_w, int nmp, const uint8_t* mp_bad, float* mp_pos,
                                   const int* mp_ref, const int* mp_by, const int* mp_cref, int loopKF, int curKF, int n_nc, const int* nc_kf, const double* nc_S, int n_c,
                                   const int* c_kf, const double* c_S, int n_lc, const int* lc_kf, const int* lc_off, const int* lc, int fix_scale, int cap_v, int cap_e,
                                   int* N_out, int* E_out, int* vertex_kf, int* edges, int* fixed_out) {
  HM_TRY(
    EssentialGraphMap map;
    map.mvpKeyFrames.resize((size_t)nkf);
    for (int i = 0; i < nkf; ++i) {
      EssGraphKeyFrameView& k = map.mvpKeyFrames[(size_t)i];
      k.mnId = (long unsigned int)mnId[i]; k.mbBad = bad[i] != 0; k.mpParent = parent[i];
      std::memcpy(k.Tcw, Tcw + 12 * (size_t)i, 48);
      k.mspChildrens.insert(child + child_off[i], child + child_off[i + 1]);
      k.mspLoopEdges.insert(loop + loop_off[i], loop + loop_off[i + 1]);
      k.mvpOrderedConnectedKeyFrames.assign(cov + cov_off[i], cov + cov_off[i + 1]);
      k.mvOrderedWeights.assign(cov_w + cov_off[i], cov_w + cov_off[i + 1]);
    }
    map.mvpMapPoints.resize((size_t)nmp);
    for (int i = 0; i < nmp; ++i) {
      EssGraphMapPointView& m = map.mvpMapPoints[(size_t)i];
      m.mbBad = mp_bad[i] != 0; m.mpRefKF = mp_ref[i]; m.mnCorrectedByKF = (long unsigned int)mp_by[i]; m.mnCorrectedReference = (long unsigned int)mp_cref[i];
      std::memcpy(m.mWorldPos, mp_pos + 3 * (size_t)i, 12);
    }
    auto poses = [](int n, const int* kf, const double* S) {
      KeyFrameAndPose m;
      for (int i = 0; i < n; ++i) { Sim3Pose p; std::memcpy(p.q, S + 8 * (size_t)i, 32); std::memcpy(p.t, S + 8 * (size_t)i + 4, 24); p.s = S[8 * (size_t)i + 7]; m[kf[i]] = p; }
      return m;
    };
    const KeyFrameAndPose nc = poses(n_nc, nc_kf, nc_S), co = poses(n_c, c_kf, c_S);
    std::map<int, std::set<int>> lcm;
    for (int i = 0; i < n_lc; ++i) lcm[lc_kf[i]].insert(lc + lc_off[i], lc + lc_off[i + 1]);
    const EssGraph g = Optimizer::CollectEssentialGraph(map, loopKF, curKF, nc, co, lcm);
    const int N = (int)g.vertexKF.size(), E = (int)g.edges.size() / 3;
    if (N > cap_v || E > cap_e) throw std::runtime_error("hm_ess_graph_mirror: the graph exceeds the caller's arrays");
    *N_out = N; *E_out = E; *fixed_out = g.fixed;
    std::memcpy(vertex_kf, g.vertexKF.data(), sizeof(int) * (size_t)N);
    std::memcpy(edges, g.edges.data(), sizeof(int) * 3 * (size_t)E);
    Optimizer::OptimizeEssentialGraph(map, loopKF, curKF, nc, co, lcm, fix_scale != 0, engine ? Optimizer::HOST_CORE : Optimizer::DEVICE);
    for (int i = 0; i < nkf; ++i) std::memcpy(Tcw + 12 * (size_t)i, map.mvpKeyFrames[(size_t)i].Tcw, 48);
    for (int i = 0; i < nmp; ++i) std::memcpy(mp_pos + 3 * (size_t)i, map.mvpMapPoints[(size_t)i].mWorldPos, 12);
    return 0;)
}

// Optimizer::GlobalBundleAdjustemnt of cubemap_hot_path.h over flat arrays.  Key frames (nkf of them, the first n_list are the call's list): mnId, bad, Tcw
// (16 floats, row-major 4x4, in/out), nkp key points each (x, y | octave | ray), one invSigma2 table.  Map points: mnId, bad, Xw (in/out), observations in CSR
// form (key-frame index, key-point index).  hm_global_ba_collect returns what CollectGlobalBA made (capacities: nkf poses, nmp points, obs_off[nmp] edges);
// hm_global_ba_mirror runs the call and hands back Tcw / Xw, and mTcwGBA / mPosGBA / mnBAGlobalForKF where the call created them (other rows untouched).
static GlobalBAMap gba_map(int nkf, int n_list, const long* kf_id, const uint8_t* kf_bad, float* Tcw, int nkp, const float* keys, const int* octave, const float* rays,
                           const float* inv_sigma2, int nlevels, int nmp, const long* mp_id, const uint8_t* mp_bad, float* Xw, const int* obs_off, const int* obs_kf,
                           const int* obs_kp) {
  GlobalBAMap map;
  map.nListedKeyFrames = n_list;
  map.mvpKeyFrames.resize((size_t)nkf);
  for (int k = 0; k < nkf; ++k) {
    GlobalBAKeyFrameView& v = map.mvpKeyFrames[(size_t)k];
    v.mnId = (long unsigned int)kf_id[k]; v.mbBad = kf_bad[k] != 0;
    v.Tcw = cv::Mat(4, 4, cv::CV_32F, Tcw + 16 * (size_t)k, 16);
    v.mvInvLevelSigma2.assign(inv_sigma2, inv_sigma2 + nlevels);
    v.mvKeys.resize((size_t)nkp); v.mvKeyRays.resize((size_t)nkp);
    for (int i = 0; i < nkp; ++i) {
      const size_t o = (size_t)k * nkp + i;
      v.mvKeys[(size_t)i].pt = cv::Point2f(keys[2 * o], keys[2 * o + 1]); v.mvKeys[(size_t)i].octave = octave[o];
      for (int c = 0; c < 3; ++c) v.mvKeyRays[(size_t)i].v[c] = rays[3 * o + c];
    }
  }
  map.mvpMapPoints.resize((size_t)nmp);
  for (int p = 0; p < nmp; ++p) {
    GlobalBAMapPointView& m = map.mvpMapPoints[(size_t)p];
    m.mnId = (long unsigned int)mp_id[p]; m.mbBad = mp_bad[p] != 0;
    m.Xw = cv::Mat(3, 1, cv::CV_32F, Xw + 3 * (size_t)p, 4);
    for (int o = obs_off[p]; o < obs_off[p + 1]; ++o) m.observations.push_back(std::make_pair(obs_kf[o], obs_kp[o]));
  }
  return map;
}
extern "C" int hm_global_ba_collect(int nkf, int n_list, const long* kf_id, const uint8_t* kf_bad, float* Tcw, int nkp, const float* keys, const int* octave,
                                    const float* rays, const float* inv_sigma2, int nlevels, int nmp, const long* mp_id, const uint8_t* mp_bad, float* Xw,
                                    const int* obs_off, const int* obs_kf, const int* obs_kp, int* KPE, int* vertex_kf, int* vertex_mp, double* poses, uint8_t* fixed,
                                    double* points, int* e_pose, int* e_point, double* e_obs, double* e_invsig2, int8_t* e_face, uint8_t* not_included) {
  HM_TRY(
    const GlobalBAMap map = gba_map(nkf, n_list, kf_id, kf_bad, Tcw, nkp, keys, octave, rays, inv_sigma2, nlevels, nmp, mp_id, mp_bad, Xw, obs_off, obs_kf, obs_kp);
    const GlobalBAGraph g = Optimizer::CollectGlobalBA(map);
    const size_t K = g.vertexKF.size(), P = g.vertexMP.size(), E = g.e_pose.size();
    KPE[0] = (int)K; KPE[1] = (int)P; KPE[2] = (int)E;
    std::memcpy(vertex_kf, g.vertexKF.data(), sizeof(int) * K); std::memcpy(vertex_mp, g.vertexMP.data(), sizeof(int) * P);
    std::memcpy(poses, g.poses.data(), sizeof(double) * 7 * K); std::memcpy(fixed, g.fixed.data(), K);
    std::memcpy(points, g.points.data(), sizeof(double) * 3 * P);
    std::memcpy(e_pose, g.e_pose.data(), sizeof(int) * E); std::memcpy(e_point, g.e_point.data(), sizeof(int) * E);
    std::memcpy(e_obs, g.e_obs.data(), sizeof(double) * 2 * E); std::memcpy(e_invsig2, g.e_invsig2.data(), sizeof(double) * E);
    std::memcpy(e_face, g.e_face.data(), E);
    std::memcpy(not_included, g.vbNotIncludedMP.data(), (size_t)nmp);
    return 0;)
}
extern "C" int hm_global_ba_mirror(int nkf, int n_list, const long* kf_id, const uint8_t* kf_bad, float* Tcw, int nkp, const float* keys, const int* octave,
                                   const float* rays, const float* inv_sigma2, int nlevels, int nmp, const long* mp_id, const uint8_t* mp_bad, float* Xw,
                                   const int* obs_off, const int* obs_kf, const int* obs_kp, int iterations, uint8_t* stop, long nLoopKF, int robust, float* TcwGBA,
                                   long* kf_gba, float* PosGBA, long* mp_gba) {
  HM_TRY(
    GlobalBAMap map = gba_map(nkf, n_list, kf_id, kf_bad, Tcw, nkp, keys, octave, rays, inv_sigma2, nlevels, nmp, mp_id, mp_bad, Xw, obs_off, obs_kf, obs_kp);
    Optimizer::GlobalBundleAdjustemnt(map, iterations, reinterpret_cast<bool*>(stop), (unsigned long)nLoopKF, robust != 0);
    for (int k = 0; k < nkf; ++k) {
      const GlobalBAKeyFrameView& v = map.mvpKeyFrames[(size_t)k];
      kf_gba[k] = (long)v.mnBAGlobalForKF;
      if (!v.mTcwGBA.empty()) for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) TcwGBA[16 * (size_t)k + 4 * r + c] = v.mTcwGBA.at<float>(r, c);
    }
    for (int p = 0; p < nmp; ++p) {
      const GlobalBAMapPointView& m = map.mvpMapPoints[(size_t)p];
      mp_gba[p] = (long)m.mnBAGlobalForKF;
      if (!m.mPosGBA.empty()) for (int c = 0; c < 3; ++c) PosGBA[3 * (size_t)p + c] = m.mPosGBA.at<float>(c, 0);
    }
    return 0;)
}
