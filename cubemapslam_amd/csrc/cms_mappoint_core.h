// cms_mappoint_core.h -- the numeric core of the resident map points: MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:243-308) and
// MapPoint::UpdateNormalAndDepth (:332-373) over the observation index of csrc/cms_covis_core.h, on plain arrays.  ONE source for the host build
// (libcubemapslam_host.so: hm_mpstore_*, the definition of record) and for the gfx950 kernels (cms_mappoint_kernels.hip).  It compiles under g++ as
// it stands; both builds use -ffp-contract=off, so every float operation below is the plain IEEE one in the order written.
//
// Observations of an id: the index's entries (member position m_k, feature f_k, octave o_k), k < N, taken in ASCENDING MEMBER POSITION.  The
// reference iterates a std::map<KeyFrame*, size_t>, so the pointer decides its order; here the earlier member position goes first, the rule of
// cms_covis_core.h.  A caller of cms_distinctive_descriptors / cms_update_normal_and_depth that lists observations in member order gets these results.
//
// Distinctive descriptor: D_k = descriptor row f_k of the slot of member m_k.  Row i of the N x N Hamming matrix (its own 0 included) is sorted, its
// median is the entry at index (int)(0.5 * (N - 1)); the result is the k of least median, the earliest k on ties (`median < BestMedian`).
// Normal and depth: k_update_normal_depth's float arithmetic (cms_tri_kernels.hip), with Ow what the store holds when the call runs and octaves and
// features the index's snapshot; the bounds come from the observation whose member's slot is the point's reference slot.
#ifndef CMS_MAPPOINT_CORE_H
#define CMS_MAPPOINT_CORE_H
#include <stdint.h>
#include "cms_covis_core.h"
#include "cms_project_helpers.h"      // tri_dnorm3

#define CMS_MP_DESCRIPTOR 1
#define CMS_MP_NORMAL_DEPTH 2
// per-id status of a refresh
#define CMS_MP_DONE 0
#define CMS_MP_NO_OBSERVATION 1      // the index knows no observation of the id: the row is untouched (the reference's early return)
#define CMS_MP_NO_REFERENCE 2        // normal and depth were asked for and the reference slot is no member that observes the id: the row is untouched

// the index of the median in a sorted row of N distances (MapPoint.cpp:296)
CMS_HD int cms_mp_median_index(int n) { return (int)(0.5 * (n - 1)); }
// one int that orders (median, earlier member position first) for a minimum: medians are at most 256, positions below 16384
CMS_HD int cms_mp_best_key(int median, int member) { return (median << 14) | member; }
CMS_HD int cms_mp_best_key_member(int key) { return key & (CMS_COVIS_MAX_MEMBERS - 1); }
// Hamming distance of two 32-byte descriptors given as eight words each
CMS_HD int cms_mp_hamming256(const uint32_t* a, const uint32_t* b) {
  int d = 0;
  for (int w = 0; w < 8; ++w) d += __builtin_popcount(a[w] ^ b[w]);
  return d;
}
// one observation into the running normal: ni = P - Ow, normal = normal * 1 + ni * (1 / |ni|)   (cv::addWeighted, MapPoint.cpp:352-356)
CMS_HD void cms_mp_normal_add(float* nrm, const float* P, const float* Ow) {
  const float ni[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
  const float beta = (float)(1.0 / tri_dnorm3(ni));
  for (int k = 0; k < 3; ++k) nrm[k] = cms_fmul_rn(nrm[k], 1.0f) + cms_fmul_rn(ni[k], beta);
}
// mNormalVector = normal / n (:371)
CMS_HD void cms_mp_normal_finish(const float* nrm, int n, float* out) {
  const float inv_n = (float)(1.0 / (double)n);
  for (int k = 0; k < 3; ++k) out[k] = cms_fmul_rn(nrm[k], inv_n);
}
// mfMaxDistance = dist * levelScaleFactor, mfMinDistance = mfMaxDistance / mvScaleFactors[nLevels - 1] (:361-370).  sf_level: the scale factor of
// the reference observation's octave, sf_top: of the last level
CMS_HD void cms_mp_bounds(const float* P, const float* Ow_ref, float sf_level, float sf_top, float* min_dist, float* max_dist) {
  const float PC[3] = {P[0] - Ow_ref[0], P[1] - Ow_ref[1], P[2] - Ow_ref[2]};
  const float dist = (float)tri_dnorm3(PC);
  const float mx = cms_fmul_rn(dist, sf_level);
  *max_dist = mx;
  *min_dist = mx / sf_top;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// host only from here: the table of record
#include <string.h>
#include <algorithm>
#include <vector>

// The store's and the table's stand-in of the host build: CmsCovisHostStore's slots (mp row, octaves) with a descriptor row and a camera centre per
// slot, the member list of the last build, and the map-point rows.  Calls return 0 or -1 (a refused call writes nothing), -3 where the C-ABI says
// CMS_ERR_UNSUPPORTED.
struct CmsMpHostStore {
  struct Row {
    uint8_t state = 0;      // 1: set, 2: has a descriptor, 4: has normal and depth
    float pos[3] = {0, 0, 0}, normal[3] = {0, 0, 0}, min_dist = 0, max_dist = 0;
    uint8_t desc[32] = {0};
    int ref = -1, best_member = -1, best_feature = -1;
    int visible = 1, found = 1, first_kf = -1;      // cms_mpstats_core.h: what both MapPoint constructors leave
  };
  CmsCovisHostStore cv;
  std::vector<std::vector<uint8_t>> desc;      // per slot: n x 32
  std::vector<float> Ow;                       // per slot: 3
  std::vector<float> Rcw, tcw, median;         // per slot: 9, 3, 1 (hm_mpstats_*: the scene median depth).  put() leaves Rcw = I, tcw = -Ow
  std::vector<int> member_slot;                // of the last successful build
  std::vector<Row> rows;
  float sf[16];
  int nlevels;

  CmsMpHostStore(int max_keyframes, int max_feat, int max_mem, int max_points, int nlev, const float* scale)
      : cv(max_keyframes, max_feat, max_mem), desc((size_t)max_keyframes), Ow((size_t)max_keyframes * 3, 0.0f), Rcw((size_t)max_keyframes * 9, 0.0f),
        tcw((size_t)max_keyframes * 3, 0.0f), median((size_t)max_keyframes, 1.0f), rows((size_t)max_points), nlevels(nlev) {
    for (int l = 0; l < 16; ++l) sf[l] = l < nlev ? scale[l] : 1.0f;
  }
  int put(int s, int n, const int* mp, const int* oct, const uint8_t* d, const float* ow) {
    if (!ow || (n > 0 && !d)) return -1;
    for (int f = 0; f < n; ++f) if (oct[f] < 0 || oct[f] >= nlevels) return -1;
    if (cv.put(s, n, mp, oct)) return -1;
    desc[(size_t)s].assign(d, d + (size_t)n * 32);
    memcpy(&Ow[(size_t)s * 3], ow, 12);
    for (int k = 0; k < 9; ++k) Rcw[(size_t)s * 9 + k] = (k % 4 == 0) ? 1.0f : 0.0f;
    for (int k = 0; k < 3; ++k) tcw[(size_t)s * 3 + k] = -ow[k];
    return 0;
  }
  int update_poses(int n, const int* slot, const float* ow) {
    for (int i = 0; i < n; ++i) if (!cv.slot_ok(slot[i]) || !cv.slots[(size_t)slot[i]].used) return -1;
    for (int i = 0; i < n; ++i) memcpy(&Ow[(size_t)slot[i] * 3], ow + 3 * (size_t)i, 12);
    return 0;
  }
  int build(int nm, const int* member_slots) {
    const int rc = cv.build(nm, member_slots);
    if (rc == 0) member_slot.assign(member_slots, member_slots + nm);
    return rc;
  }
  bool id_ok(int id) const { return id >= 0 && (size_t)id < rows.size(); }
  // an id out of range or named twice?
  bool ids_ok(int n, const int* ids) const {
    std::vector<int> s(ids, ids + n);
    std::sort(s.begin(), s.end());
    for (int i = 0; i < n; ++i) if (!id_ok(s[(size_t)i]) || (i > 0 && s[(size_t)i] == s[(size_t)i - 1])) return false;
    return true;
  }
  int set(int n, const int* ids, const float* pos, const int* ref_slot) {
    if (n < 0 || (n > 0 && !ids) || !ids_ok(n, ids)) return -1;
    for (int i = 0; i < n; ++i) {
      if (!(rows[(size_t)ids[i]].state & 1) && (!pos || !ref_slot)) return -1;      // a new row wants both
      if (ref_slot && !cv.slot_ok(ref_slot[i])) return -1;
    }
    for (int i = 0; i < n; ++i) {
      Row& r = rows[(size_t)ids[i]];
      if (pos) memcpy(r.pos, pos + 3 * (size_t)i, 12);
      if (ref_slot) r.ref = ref_slot[i];
      r.state |= 1;
    }
    return 0;
  }
  int erase(int n, const int* ids) {
    if (n < 0 || (n > 0 && !ids) || !ids_ok(n, ids)) return -1;
    for (int i = 0; i < n; ++i) rows[(size_t)ids[i]] = Row();
    return 0;
  }
  int refresh(int n, const int* ids, int what, uint8_t* status) {
    if (n < 0 || (n > 0 && (!ids || !status)) || what < 1 || what > 3 || !ids_ok(n, ids)) return -1;
    for (int i = 0; i < n; ++i) if (!(rows[(size_t)ids[i]].state & 1)) return -1;
    const CmsCovisHost& ix = cv.index;
    for (int i = 0; i < n; ++i) {
      Row& r = rows[(size_t)ids[i]];
      const int u = ix.find(ids[i]);
      if (u < 0) { status[i] = CMS_MP_NO_OBSERVATION; continue; }
      const CmsCovisHost::Obs* o = &ix.obs[(size_t)ix.seg[(size_t)u]];      // sorted by member
      const int N = ix.seg[(size_t)u + 1] - ix.seg[(size_t)u];
      int kref = -1;
      for (int k = 0; k < N; ++k) if (member_slot[(size_t)o[k].member] == r.ref) kref = k;
      if ((what & CMS_MP_NORMAL_DEPTH) && kref < 0) { status[i] = CMS_MP_NO_REFERENCE; continue; }
      if (what & CMS_MP_DESCRIPTOR) {
        std::vector<uint32_t> D((size_t)N * 8);
        for (int k = 0; k < N; ++k) memcpy(&D[(size_t)k * 8], &desc[(size_t)member_slot[(size_t)o[k].member]][(size_t)o[k].feat * 32], 32);
        int best = 0x7FFFFFFF;
        std::vector<int> row((size_t)N);
        for (int a = 0; a < N; ++a) {
          for (int b = 0; b < N; ++b) row[(size_t)b] = cms_mp_hamming256(&D[(size_t)a * 8], &D[(size_t)b * 8]);
          std::sort(row.begin(), row.end());
          best = std::min(best, cms_mp_best_key(row[(size_t)cms_mp_median_index(N)], o[a].member));
        }
        for (int k = 0; k < N; ++k)
          if (o[k].member == cms_mp_best_key_member(best)) { memcpy(r.desc, &D[(size_t)k * 8], 32); r.best_member = o[k].member; r.best_feature = o[k].feat; }
        r.state |= 2;
      }
      if (what & CMS_MP_NORMAL_DEPTH) {
        float nrm[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < N; ++k) cms_mp_normal_add(nrm, r.pos, &Ow[(size_t)member_slot[(size_t)o[k].member] * 3]);
        cms_mp_normal_finish(nrm, N, r.normal);
        cms_mp_bounds(r.pos, &Ow[(size_t)r.ref * 3], sf[o[kref].octave], sf[nlevels - 1], &r.min_dist, &r.max_dist);
        r.state |= 4;
      }
      status[i] = CMS_MP_DONE;
    }
    return 0;
  }
  int fetch(int n, const int* ids, float* pos, float* normal, float* min_dist, float* max_dist, uint8_t* d, int* best_member, int* best_feature) const {
    for (int i = 0; i < n; ++i) if (!id_ok(ids[i])) return -1;
    for (int i = 0; i < n; ++i) {
      const Row& r = rows[(size_t)ids[i]];
      if (pos) memcpy(pos + 3 * (size_t)i, r.pos, 12);
      if (normal) memcpy(normal + 3 * (size_t)i, r.normal, 12);
      if (min_dist) min_dist[i] = r.min_dist;
      if (max_dist) max_dist[i] = r.max_dist;
      if (d) memcpy(d + 32 * (size_t)i, r.desc, 32);
      if (best_member) best_member[i] = r.best_member;
      if (best_feature) best_feature[i] = r.best_feature;
    }
    return 0;
  }
};
#endif
