// cms_sim3_search_core.h -- the arithmetic of ORBMatcher::SearchBySim3 (src/ORBMatcher.cpp:1365-1586) in front of its window query: the composition
// of the similarity (:1377-1379) and, for one direction, the chain from a map point's world position to (u, v, dist3D, why it is dropped)
// (:1416-1442 and :1497-1523).  ONE source for the host build (libcubemapslam_host.so: hm_sim3s_compose, hm_sim3s_project) and for the gfx950 kernel
// (k_sim3s_project, cms_sim3_search_kernels.hip); the host side of cms_kfstore_search_by_sim3 composes each job's similarity through it as well.
// Compiles under g++ as it stands.  Plain IEEE operations in the order this source fixes; both builds use -ffp-contract=off.
//
// Expressions whose shape the project fixed before keep that convention -- the chain calls the helpers the Fuse kernel (k_fuse_project) calls:
//   R*x + t      tri_mat3_vec: float products summed left to right, then (float)((double)sum * 1.0 + (double)t * 1.0)
//   cv::norm     tri_dnorm3: sqrt of the double sum of double squares; narrowed by the caller
//   distances    track_distance_bounds: Get{Min,Max}DistanceInvariance and mfMaxDistance from what cms_set_distance_bounds_mode says was handed over
//   projection   track_rays_to_cubemap (cms_cubemap_project.h)
// The first three live in cms_project_helpers.h, one CMS_HD definition each for both builds; tests/test_sim3_search_cpu.py holds the host build to
// the numpy restatement bit for bit and tests/test_gpu_search_by_sim3.py holds the device to the same restatement.
//
// Three expressions are new here; one stated choice each (DESIGN.md "SearchBySim3 on the device"):
//   s12 * R12              float scalar times CV_32F matrix: one float multiply per element
//   (1.0 / s12) * R12.t()  the scalar is 1.0 / (double)s12 narrowed to float once; each element of the transpose takes one float multiply by it
//   -sR21 * t12            per row the double sum of the double products, k upwards from 0.0, negated, narrowed once (as Ow = -Rcw.t()*tcw elsewhere)
//
// One stated difference from the reference: where TransformRaysToCubemap answers UNKNOWN_FACE -- no face claims the ray, or the pixel rounds onto
// the far edge of its face -- the reference's assert aborts (or, compiled out, the search goes on with a face-local pixel).  Here u = v = -1 and the
// point is dropped by the IsInImage test.  With the depth of line :1507 as written (z = y) every point with y > 0 and |x| <= y lands on that edge
// (vp == F) and is dropped this way.
#ifndef CMS_SIM3_SEARCH_CORE_H
#define CMS_SIM3_SEARCH_CORE_H
#include "cms_project_helpers.h"      // CMS_HD, tri_*, track_distance_bounds, track_rays_to_cubemap = CamModelGeneral::TransformRaysToCubemap

#define CMS_SIM3S_KEEP 0
#define CMS_SIM3S_BEHIND 1      /* z < 0 (:1421, :1502) */
#define CMS_SIM3S_IMAGE 2       /* unknown face or !IsInImage (:1433, :1514) */
#define CMS_SIM3S_DIST 3        /* outside the scale-invariance distances (:1441, :1522) */

// sR12 | t12 carry key frame 2's camera frame into key frame 1's, sR21 | t21 the other way (row major)
struct CmsSim3sMotion { float sR12[9], t12[3], sR21[9], t21[3]; };

CMS_HD void cms_sim3s_compose(float s12, const float* R12, const float* t12, CmsSim3sMotion* m) {
  for (int i = 0; i < 9; ++i) m->sR12[i] = s12 * R12[i];                        // cv::Mat sR12 = s12*R12;
  const float inv = (float)(1.0 / (double)s12);                                  // cv::Mat sR21 = (1.0/s12)*R12.t();
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) m->sR21[3 * r + c] = inv * R12[3 * c + r];
  for (int r = 0; r < 3; ++r) {                                                  // cv::Mat t21 = -sR21*t12;
    double s = 0.0;
    for (int k = 0; k < 3; ++k) s = s + (double)m->sR21[3 * r + k] * (double)t12[k];
    m->t21[r] = (float)(-1.0 * s);
    m->t12[r] = t12[r];
  }
}

// One direction for one map point: Pw through its own key frame's pose (Rw | tw), then through the similarity (sR | t) into the other camera.
// second_as_depth != 0: the ray handed to the projection is (x, y, y), line :1507 as written; the depth test and dist3D use the true vector.
// u, v = -1 unless the point reaches the distance test; dist3D and raw_max (mfMaxDistance, PredictScale's numerator) are always written.
CMS_HD int cms_sim3s_project(int F, const float* Rw, const float* tw, const float* sR, const float* t, const float* Pw, int second_as_depth,
                             int bounds_scaled, float min_in, float max_in, float* u, float* v, float* dist3D, float* raw_max) {
  float pa[3], pb[3];
  tri_mat3_vec(Rw, Pw, tw, pa);                      // p3Dc1 = R1w*p3Dw + t1w   (p3Dc2 = R2w*p3Dw + t2w)
  tri_mat3_vec(sR, pa, t, pb);                       // p3Dc2 = sR21*p3Dc1 + t21 (p3Dc1 = sR12*p3Dc2 + t12)
  float minDistance, maxDistance, maxd;
  track_distance_bounds(bounds_scaled, min_in, max_in, minDistance, maxDistance, maxd);
  const float d = (float)tri_dnorm3(pb);
  *u = -1.0f; *v = -1.0f; *dist3D = d; *raw_max = maxd;
  if (pb[2] < 0.0f) return CMS_SIM3S_BEHIND;
  float uu = -1.0f, vv = -1.0f;
  if (track_rays_to_cubemap(F, pb[0], pb[1], second_as_depth ? pb[1] : pb[2], uu, vv) < 0) { uu = -1.0f; vv = -1.0f; }
  const float mx = (float)(3 * F);
  if (!(uu >= 0.0f && uu < mx && vv >= 0.0f && vv < mx)) return CMS_SIM3S_IMAGE;      // KeyFrame::IsInImage
  *u = uu; *v = vv;
  if (d < minDistance || d > maxDistance) return CMS_SIM3S_DIST;
  return CMS_SIM3S_KEEP;
}

#endif
