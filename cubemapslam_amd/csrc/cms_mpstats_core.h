// cms_mpstats_core.h -- the rules of the map-point statistics: the verdict of LocalMapping::MapPointCulling (src/LocalMapping.cpp:187-204), the depth of
// KeyFrame::ComputeSceneMedianDepth (src/KeyFrame.cpp:1086) and the order in which its depths are ranked (:1091-1093).  ONE source for the host build
// (libcubemapslam_host.so: hm_mpstats_*, the definition of record) and for the gfx950 kernels (cms_mpstats_kernels.hip).  It compiles under g++ as it
// stands; both builds use -ffp-contract=off, so every float operation below is the plain IEEE one in the order written.
#ifndef CMS_MPSTATS_CORE_H
#define CMS_MPSTATS_CORE_H
#include <stdint.h>
#include <string.h>
#include "cms_project_helpers.h"      // CMS_HD, tri_ddot3

#define CMS_MP_VISIBLE 1      // Tracking.cpp:808 and :829: IncreaseVisible()
#define CMS_MP_FOUND 2        // Tracking.cpp:698 (and :264): IncreaseFound()

// per-id verdict of a culling call
#define CMS_MP_STAYS 0            // stays in mlpRecentAddedMapPoints
#define CMS_MP_BAD_RATIO 1        // GetFoundRatio() < 0.25f: SetBadFlag
#define CMS_MP_BAD_FEW_OBS 2      // two key frames on and no more than th_obs observations: SetBadFlag
#define CMS_MP_LEAVES 3           // three key frames on: leaves the list alive
#define CMS_MP_ALREADY_BAD 4      // the row is empty (isBad(), :187); the entry reports it, the core never sees the case

// what an empty row holds: both MapPoint constructors leave mnVisible = mnFound = 1 (MapPoint.cpp:38-41, :53-57); no first key frame
#define CMS_MP_EMPTY_VISIBLE 1
#define CMS_MP_EMPTY_FOUND 1
#define CMS_MP_EMPTY_FIRST_KF (-1)

// the if / else if chain of LocalMapping.cpp:187-204.  GetFoundRatio (MapPoint.cpp:235-239) is one float division of the two converted ints; the
// key-frame ids are subtracted as ints (:196, :201; the difference wraps instead of overflowing)
CMS_HD int cms_mpstats_verdict(int found, int visible, int first_kf, int n_obs, int current_kf, int th_obs) {
  const float ratio = (float)found / (float)visible;
  if (ratio < 0.25f) return CMS_MP_BAD_RATIO;
  const int age = (int)((uint32_t)current_kf - (uint32_t)first_kf);
  if (age >= 2 && n_obs <= th_obs) return CMS_MP_BAD_FEW_OBS;
  if (age >= 3) return CMS_MP_LEAVES;
  return CMS_MP_STAYS;
}

// Rcw2.dot(x3Dw) + zcw (KeyFrame.cpp:1086): Mat::dot is the double sum of double products in component order, zcw joins in double, and the
// assignment to a float narrows once -- cms_tri_kernels.hip's third camera coordinate
CMS_HD float cms_mpstats_depth(const float* Rcw, const float* tcw, const float* X) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (float)__dadd_rn(tri_ddot3(Rcw + 6, X), (double)tcw[2]);
#else
  return (float)(tri_ddot3(Rcw + 6, X) + (double)tcw[2]);
#endif
}

// A monotone integer image of a float: the sign bit flipped for non-negative values, all bits for negative ones, so -0.0f orders before +0.0f.
// "Element idx of the sorted depths" is the smallest key v with #(key <= v) > idx, decoded: no sort, and no freedom of a comparator.  The value
// equals what std::sort leaves at that index
CMS_HD uint32_t cms_mpstats_depth_key(float z) {
  uint32_t u;
  memcpy(&u, &z, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
CMS_HD float cms_mpstats_depth_from_key(uint32_t key) {
  const uint32_t u = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
  float z;
  memcpy(&z, &u, 4);
  return z;
}
// the index ComputeSceneMedianDepth reads in n sorted depths (:1093); n >= 1, q >= 1
CMS_HD int cms_mpstats_depth_index(int n, int q) { return (n - 1) / q; }
#endif
