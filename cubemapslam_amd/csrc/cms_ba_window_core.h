// cms_ba_window_core.h -- the window of Optimizer::LocalBundleAdjustment (src/Optimizer.cpp:194-357) assembled from the observation index of
// csrc/cms_covis_core.h, the store's slots and the map-point table, on plain arrays.  ONE source for the host build (libcubemapslam_host.so:
// hm_ba_window_build, the definition of record) and for the gfx950 kernels (cms_ba_window_kernels.hip).  It compiles under g++ as it stands; both
// builds use -ffp-contract=off, and nothing below has a multiply next to an add that a contraction could join.
//
// A job is { n_local, local_members[], first_member }: lLocalKeyFrames in the reference's order (the current key frame, then its
// GetVectorCovisibleKeyFrames(), the `order` of cms_covis_connections) as member POSITIONS of the index, and the member whose mnId is 0 (-1: none,
// :268).  Members of the index are not bad by definition.
//
//   local points (:209-225)   the ids of the local members' rows in list order, then feature order, each at its first occurrence:
//                             CmsCovisHost::local_points of the same list.  point_id[p], p < P
//   fixed key frames (:227-243)   every member that is not local and observes a local point.  The reference walks lLocalMapPoints in list order and,
//                             inside a point, its std::map<KeyFrame*, size_t> of observations -- ascending member position here, the rule of
//                             cms_covis_core.h -- and pushes a key frame when it meets it for the first time (mnBAFixedForKF).  A member m that is
//                             first met at point first(m) is pushed before every member first met at a later point, and among the members first met
//                             at the same point the walk reaches the lower position first.  Hence lFixedCameras is the fixed members in ascending
//                             (first(m), m): one sort by a key, no walk (cms_baw_fixed_key: 64 bits, first(m) alone may pass 2^17)
//   window key frames         kf_member[k]: the locals in list order (k < n_local), then the fixed ones; K of them.
//                             fixed[k] = k >= n_local || kf_member[k] == first_member (:268, :281)
//   poses (:266, :279)        Converter::toSE3Quat (Converter.cpp:41-51): the slot's float Rcw and tcw widened to double, poses[7k ..] = (t, q) with
//                             q = Eigen::Quaterniond(Matrix3d) (cms_baw_quat)
//   points (:306)             points[3p ..]: the table's float position widened to double
//   edges (:312-356)          p in list order, the observations of point_id[p] in ascending member position.  One whose key ray has z < cos_fov
//                             (float, :323-325) or whose key point lies on no face (the mirror's rule: g2o would exit) is skipped; the others give
//                             e_pose (the window index of the member), e_point = p, e_obs = GetPosInFace<double>, e_face, e_invsig2 = (double)
//                             mvInvLevelSigma2[octave] with the index's octave, e_feat = the feature index.  A point that loses all its edges stays
//                             in the list: the reference adds its vertex
// The outputs are counts = {K, n_local, P, E} and the arrays, in the layout of cms_ba_create's arguments.
#ifndef CMS_BA_WINDOW_CORE_H
#define CMS_BA_WINDOW_CORE_H
#include <math.h>
#include <stdint.h>
#include "cms_covis_core.h"
#include "cms_sim3_opt_core.h"      // cms_s3o_face_in_cubemap, cms_s3o_pos_in_face

typedef struct { int K, n_local, P, E; } CmsBaWindowCounts;      // cms_ba_window_counts of the C-ABI

// the place of a fixed member in lFixedCameras: ascending (list position of the first local point it observes, member position)
CMS_HD unsigned long long cms_baw_fixed_key(int first_point, int member) { return ((unsigned long long)(unsigned)first_point << 14) | (unsigned long long)(unsigned)member; }
CMS_HD bool cms_baw_is_fixed(int k, int n_local, int member, int first_member) { return k >= n_local || member == first_member; }

// Eigen::Quaterniond(Matrix3d) on a row-major m, q = (x, y, z, w): R_to_quat of host/cubemap_hot_path.cpp
CMS_HD void cms_baw_quat(const double* m, double* q) {
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + 1.0);
    const double qi = 0.5 * t;
    t = 0.5 / t;
    const double qw = (m[k * 3 + j] - m[j * 3 + k]) * t, qj = (m[j * 3 + i] + m[i * 3 + j]) * t, qk = (m[k * 3 + i] + m[i * 3 + k]) * t;
    // (written through selects, not q[i]: a runtime index would put the kernel's q into scratch memory)
    q[0] = i == 0 ? qi : (j == 0 ? qj : qk);
    q[1] = i == 1 ? qi : (j == 1 ? qj : qk);
    q[2] = i == 2 ? qi : (j == 2 ? qj : qk);
    q[3] = qw;
  }
}
// Converter::toSE3Quat: float Rcw (row-major), tcw -> (t, q)
CMS_HD void cms_baw_pose(const float* Rcw, const float* tcw, double* pose7) {
  double R[9];
  for (int i = 0; i < 9; ++i) R[i] = (double)Rcw[i];
  for (int i = 0; i < 3; ++i) pose7[i] = (double)tcw[i];
  cms_baw_quat(R, pose7 + 3);
}
// does the observation give an edge?  Its face, or -1: skipped by the ray test or for lying on no face
CMS_HD int cms_baw_edge_face(int F, float cos_fov, float kx, float ky, float ray_z) {
  if (ray_z < cos_fov) return -1;
  return cms_s3o_face_in_cubemap(F, kx, ky);
}
CMS_HD void cms_baw_edge_obs(int F, float kx, float ky, double* uv) { uv[0] = cms_s3o_pos_in_face(F, kx); uv[1] = cms_s3o_pos_in_face(F, ky); }

// ---------------------------------------------------------------------------------------------------------------------------------------------
// host only from here: the window of record
#include <algorithm>
#include <string>
#include <vector>

// what the walk reads besides the index: per member the key points, the rays' z and the pose of its slot; per id the table's position
struct CmsBaWindowHostData {
  int F = 0; float cos_fov = 0.0f;
  float inv_sigma2[16];
  std::vector<std::vector<float>> kx, ky, ray_z;      // per member, per feature
  std::vector<float> Rcw, tcw;                        // per member: 9, 3
  std::vector<uint8_t> has_pos;                       // per id of the table
  std::vector<float> pos;                             // per id: 3
};
struct CmsBaWindowHostJob { int n_local; const int* local_members; int first_member; };
struct CmsBaWindowHostOut {
  int cap_kf, cap_points, cap_edges;
  CmsBaWindowCounts* counts;
  int* kf_member; int* point_id; double* poses; uint8_t* fixed; double* points;
  int* e_pose; int* e_point; double* e_obs; double* e_invsig2; int8_t* e_face; int* e_feat;
};

// 0, -1 (a refused call: nothing is written; `why` says what) or -4 (CMS_ERR_OVERFLOW: every job's counts are delivered, a job that fits is
// complete, of one that does not the entries below the caps are written)
static inline int cms_ba_window_host(const CmsCovisHost& ix, const CmsBaWindowHostData& D, int njobs, const CmsBaWindowHostJob* jobs, const CmsBaWindowHostOut& o,
                                     std::string* why) {
  const int M = ix.n_members;
  auto fail = [&](const std::string& s) { if (why) *why = s; return -1; };
  if (njobs < 0 || (njobs > 0 && !jobs)) return fail("bad argument");
  if (o.cap_kf < 1 || o.cap_points < 1 || o.cap_edges < 1) return fail("a cap below 1");
  for (int j = 0; j < njobs; ++j) {
    if (jobs[j].n_local < 1 || !jobs[j].local_members) return fail("a job without a local key frame");
    if (jobs[j].first_member < -1 || jobs[j].first_member >= M) return fail("first_member names no member");
    std::vector<uint8_t> seen((size_t)M, 0);
    for (int k = 0; k < jobs[j].n_local; ++k) {
      const int m = jobs[j].local_members[k];
      if (m < 0 || m >= M) return fail("a job names no member");
      if (seen[(size_t)m]) return fail("a job names a member twice");
      seen[(size_t)m] = 1;
    }
  }
  // the local points of every job, and the rows of the table behind them, before anything is written
  std::vector<std::vector<int>> pid((size_t)njobs);
  for (int j = 0; j < njobs; ++j) {
    const int off[2] = {0, jobs[j].n_local};
    size_t bound = 1;
    for (int k = 0; k < jobs[j].n_local; ++k) bound += ix.mp[(size_t)jobs[j].local_members[k]].size();
    pid[(size_t)j].resize(bound);
    int n = 0;
    if (ix.local_points(1, off, jobs[j].local_members, (int)bound, pid[(size_t)j].data(), &n)) return fail("the local points could not be listed");
    pid[(size_t)j].resize((size_t)n);
    for (int id : pid[(size_t)j])
      if ((size_t)id >= D.has_pos.size() || !D.has_pos[(size_t)id]) return fail("job " + std::to_string(j) + ": local point " + std::to_string(id) + " has no position in the table");
  }
  bool overflow = false;
  for (int j = 0; j < njobs; ++j) {
    const CmsBaWindowHostJob& J = jobs[j];
    const std::vector<int>& ids = pid[(size_t)j];
    const int P = (int)ids.size(), nl = J.n_local;
    std::vector<int> widx((size_t)M, -1), first((size_t)M, -1);
    for (int k = 0; k < nl; ++k) widx[(size_t)J.local_members[k]] = k;
    std::vector<int> seg0((size_t)P), seg1((size_t)P);
    for (int p = 0; p < P; ++p) {
      const int u = ix.find(ids[(size_t)p]);
      seg0[(size_t)p] = ix.seg[(size_t)u]; seg1[(size_t)p] = ix.seg[(size_t)u + 1];
      for (int e = seg0[(size_t)p]; e < seg1[(size_t)p]; ++e) {
        const int m = ix.obs[(size_t)e].member;
        if (widx[(size_t)m] < 0 && first[(size_t)m] < 0) first[(size_t)m] = p;      // (p ascends: the first is the least)
      }
    }
    std::vector<unsigned long long> keys;
    for (int m = 0; m < M; ++m) if (first[(size_t)m] >= 0) keys.push_back(cms_baw_fixed_key(first[(size_t)m], m));
    std::sort(keys.begin(), keys.end());
    const int K = nl + (int)keys.size();
    for (size_t i = 0; i < keys.size(); ++i) widx[(size_t)(keys[i] & (CMS_COVIS_MAX_MEMBERS - 1))] = nl + (int)i;
    for (int k = 0; k < K && k < o.cap_kf; ++k) {
      const int m = k < nl ? J.local_members[k] : (int)(keys[(size_t)(k - nl)] & (CMS_COVIS_MAX_MEMBERS - 1));
      const size_t at = (size_t)j * (size_t)o.cap_kf + (size_t)k;
      o.kf_member[at] = m;
      o.fixed[at] = cms_baw_is_fixed(k, nl, m, J.first_member) ? 1 : 0;
      cms_baw_pose(&D.Rcw[9 * (size_t)m], &D.tcw[3 * (size_t)m], o.poses + 7 * at);
    }
    int E = 0;
    for (int p = 0; p < P; ++p) {
      const int id = ids[(size_t)p];
      if (p < o.cap_points) {
        const size_t at = (size_t)j * (size_t)o.cap_points + (size_t)p;
        o.point_id[at] = id;
        for (int c = 0; c < 3; ++c) o.points[3 * at + (size_t)c] = (double)D.pos[3 * (size_t)id + (size_t)c];
      }
      for (int e = seg0[(size_t)p]; e < seg1[(size_t)p]; ++e) {      // (a segment of the host index is sorted by member)
        const CmsCovisHost::Obs& ob = ix.obs[(size_t)e];
        const size_t m = (size_t)ob.member, f = (size_t)ob.feat;
        const int face = cms_baw_edge_face(D.F, D.cos_fov, D.kx[m][f], D.ky[m][f], D.ray_z[m][f]);
        if (face < 0) continue;
        if (E < o.cap_edges) {
          const size_t at = (size_t)j * (size_t)o.cap_edges + (size_t)E;
          o.e_pose[at] = widx[m]; o.e_point[at] = p; o.e_face[at] = (int8_t)face; o.e_feat[at] = ob.feat;
          cms_baw_edge_obs(D.F, D.kx[m][f], D.ky[m][f], o.e_obs + 2 * at);
          o.e_invsig2[at] = (double)D.inv_sigma2[ob.octave & 15];
        }
        ++E;
      }
    }
    o.counts[j] = CmsBaWindowCounts{K, nl, P, E};
    overflow = overflow || K > o.cap_kf || P > o.cap_points || E > o.cap_edges;
  }
  return overflow ? -4 : 0;
}
#endif
