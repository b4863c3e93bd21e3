// cms_sim3_proj_core.h -- the arithmetic of ORBMatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (src/ORBMatcher.cpp:796-903) and
// of ORBMatcher::Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (:1246-1363) in front of their window query: the decomposition of Scw (:799-803
// and :1249-1253) and the chain from a map point's world position to (u, v, predicted level, radius, why it is dropped) (:817-860 and :1268-1312),
// which the two functions share word for word.  ONE source for the host build (libcubemapslam_host.so: hm_sim3p_decompose, hm_sim3p_project) and for
// the gfx950 kernel (k_sim3p_project, cms_sim3_proj_kernels.hip); the host side of the two C-ABI entries decomposes each job's Scw through it as
// well.  Compiles under g++ as it stands.  Plain IEEE operations in the order this source fixes; both builds use -ffp-contract=off.
//
// The chain calls the helpers k_fuse_project calls (tri_mat3_vec, tri_dnorm3, tri_ddot3, track_distance_bounds, track_predict_scale,
// track_rays_to_cubemap): one CMS_HD definition each for both builds (cms_project_helpers.h, cms_cubemap_project.h).
//
// Three expressions are new here; one stated choice each (DESIGN.md "SearchByProjection / Fuse under a Sim3"), on the row-major 3 x 4 [sR | t]:
//   scw = sqrt(sRcw.row(0).dot(sRcw.row(0)))   the double sum of the double products, k upwards from 0.0; sqrt in double; narrowed to float once
//   Rcw = sRcw / scw, tcw = t / scw            the scalar is (float)(1.0 / (double)scw); one float multiply per element (the project's
//                                              (1.0 / s12) * R12.t() convention, cms_sim3_search_core.h)
//   Ow = -Rcw.t() * tcw                        per row the double sum of the double products, k upwards from 0.0, negated, narrowed once
//
// One stated difference from the reference, the one cms_sim3_search_core.h makes: where TransformRaysToCubemap answers UNKNOWN_FACE the reference's
// assert (:836, :1287) aborts; here u = v = -1 and the point is dropped by the IsInImage test.
#ifndef CMS_SIM3_PROJ_CORE_H
#define CMS_SIM3_PROJ_CORE_H
#include "cms_project_helpers.h"

#define CMS_SIM3P_KEEP 0
#define CMS_SIM3P_BEHIND 1      /* z < 0 (:827, :1278) */
#define CMS_SIM3P_IMAGE 2       /* unknown face or !IsInImage (:839, :1290) */
#define CMS_SIM3P_DIST 3        /* outside the scale-invariance distances (:848, :1299) */
#define CMS_SIM3P_ANGLE 4       /* PO.dot(Pn) < 0.5 * dist (:854, :1305) */

struct CmsSim3pPose { float Rcw[9], tcw[3], Ow[3], scw; };

// Scw: rows 0..2 of the 4 x 4 [sR | t], row major
CMS_HD void cms_sim3p_decompose(const float* Scw, CmsSim3pPose* p) {
  double d = 0.0;                                                                // const float scw = sqrt(sRcw.row(0).dot(sRcw.row(0)));
  for (int k = 0; k < 3; ++k) d = d + (double)Scw[k] * (double)Scw[k];
  const float scw = (float)sqrt(d);
  p->scw = scw;
  const float inv = (float)(1.0 / (double)scw);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) p->Rcw[3 * r + c] = Scw[4 * r + c] * inv;        // cv::Mat Rcw = sRcw/scw;
    p->tcw[r] = Scw[4 * r + 3] * inv;                                            // cv::Mat tcw = Scw.rowRange(0,3).col(3)/scw;
  }
  for (int r = 0; r < 3; ++r) {                                                  // cv::Mat Ow = -Rcw.t()*tcw;
    double s = 0.0;
    for (int k = 0; k < 3; ++k) s = s + (double)p->Rcw[3 * k + r] * (double)p->tcw[k];
    p->Ow[r] = (float)(-1.0 * s);
  }
}

// One map point through the decomposed similarity.  u, v = -1 unless the point reaches the distance test; level = -1 and radius = -1 unless it is
// kept; dist is always written.  sf: mvScaleFactors.
CMS_HD int cms_sim3p_project(int F, const CmsSim3pPose* ps, const float* Pw, const float* Pn, int bounds_scaled, float min_in, float max_in, float th,
                             float log_scale, int nlevels, const float* sf, float* u, float* v, float* dist, int* level, float* radius) {
  float pc[3];
  tri_mat3_vec(ps->Rcw, Pw, ps->tcw, pc);                                        // p3Dc = Rcw*p3Dw+tcw
  const float PO[3] = {Pw[0] - ps->Ow[0], Pw[1] - ps->Ow[1], Pw[2] - ps->Ow[2]}; // PO = p3Dw-Ow
  const float d = (float)tri_dnorm3(PO);
  *u = -1.0f; *v = -1.0f; *dist = d; *level = -1; *radius = -1.0f;
  if (pc[2] < 0.0f) return CMS_SIM3P_BEHIND;
  float uu = -1.0f, vv = -1.0f;
  if (track_rays_to_cubemap(F, pc[0], pc[1], pc[2], uu, vv) < 0) { uu = -1.0f; vv = -1.0f; }
  const float mx = (float)(3 * F);
  if (!(uu >= 0.0f && uu < mx && vv >= 0.0f && vv < mx)) return CMS_SIM3P_IMAGE;      // KeyFrame::IsInImage
  *u = uu; *v = vv;
  float minDistance, maxDistance, maxd;
  track_distance_bounds(bounds_scaled, min_in, max_in, minDistance, maxDistance, maxd);
  if (d < minDistance || d > maxDistance) return CMS_SIM3P_DIST;
  if (tri_ddot3(PO, Pn) < 0.5 * (double)d) return CMS_SIM3P_ANGLE;
  const int ns = track_predict_scale(maxd, d, log_scale, nlevels);
  *level = ns; *radius = th * sf[ns];
  return CMS_SIM3P_KEEP;
}

#endif
