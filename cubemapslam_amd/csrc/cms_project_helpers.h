// cms_project_helpers.h -- the small arithmetic every "map point into a key frame" chain shares: cv::Mat's 3 x 3 products and norms as the project
// fixed them, a map point's scale-invariance distances and MapPoint::PredictScale.  One source for the gfx950 kernels
// (cms_track_kernels.hip, cms_tri_kernels.hip and the Sim3 cores they include) and for the host build of those cores (libcubemapslam_host.so).
// Compiles under hipcc and under g++ as it stands: plain IEEE operations in the order this source fixes; both builds use -ffp-contract=off.
#ifndef CMS_PROJECT_HELPERS_H
#define CMS_PROJECT_HELPERS_H
#include <math.h>
#include <string.h>
#include "cms_cubemap_project.h"      // CMS_HD, track_rays_to_cubemap

CMS_HD float tri_gemm3(float a0, float a1, float a2, float b0, float b1, float b2) {   // cv::gemm small path: float, left to right
  float t = a0 * b0;
  t = t + a1 * b1;
  return t + a2 * b2;
}
CMS_HD double tri_ddot3(const float* a, const float* b) {      // Mat::dot: double sum of double products
  double s = (double)a[0] * (double)b[0];
  s = s + (double)a[1] * (double)b[1];
  return s + (double)a[2] * (double)b[2];
}
CMS_HD double tri_dnorm3(const float* a) { return sqrt(tri_ddot3(a, a)); }      // cv::norm; narrowed by the caller
CMS_HD void tri_mat3_vec(const float* A, const float* x, const float* c, float* out) {      // A*x (+ c through double: cv::gemm's C operand)
  for (int r = 0; r < 3; ++r) {
    const float t = tri_gemm3(A[3 * r], A[3 * r + 1], A[3 * r + 2], x[0], x[1], x[2]);
    out[r] = c ? (float)((double)t * 1.0 + (double)c[r] * 1.0) : t;
  }
}

// a * b rounded to nearest, unfused.  The device side keeps the intrinsic spelling: the gfx950 compiler schedules k_in_frustum and k_project_keyframe
// differently around the plain product (profiles/window_scan_refactor.md); the value is the same IEEE product either way
CMS_HD float cms_fmul_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(a, b);
#else
  return a * b;
#endif
}
CMS_HD float cms_float_step(float r, int step) {      // the float `step` representations away from r
  unsigned u;
  memcpy(&u, &r, 4);
  u += (unsigned)step;
  memcpy(&r, &u, 4);
  return r;
}
// Scale-invariance bounds of a map point (MapPoint.cpp:375-385) and mfMaxDistance itself, from what the caller handed over
// (cms_set_distance_bounds_mode): the raw members, or the public getters' values.  Handed the getters' values, the bounds are used as they are
// and mfMaxDistance is recovered as the float r with 1.2f * r == bound (the product rounds up to two neighbouring r onto one bound when it
// crosses a power of two; the smaller one is taken -- PredictScale can then differ from the reference only where log(ratio) / log(scale factor)
// sits within an ulp of an integer)
CMS_HD void track_distance_bounds(int scaled, float min_in, float max_in, float& minDistance, float& maxDistance, float& raw_max) {
  if (scaled) {
    maxDistance = max_in; minDistance = min_in;
    float r = (float)((double)max_in / (double)1.2f);
    const float lo = cms_float_step(r, -1), hi = cms_float_step(r, 1);
    if (r > 0.0f && cms_fmul_rn(1.2f, lo) == max_in) r = lo;
    else if (cms_fmul_rn(1.2f, r) != max_in && cms_fmul_rn(1.2f, hi) == max_in) r = hi;
    raw_max = r;
  } else {
    raw_max = max_in; maxDistance = cms_fmul_rn(1.2f, max_in); minDistance = cms_fmul_rn(0.8f, min_in);
  }
}
// MapPoint::PredictScale (MapPoint.cpp:404-419): ceil(logf(ratio) / mfLogScaleFactor); the float log is taken as the rounded double log (glibc's
// logf is within 0.82 ulp of it; the two can only part where the quotient sits within an ulp of an integer)
CMS_HD int track_predict_scale(float raw_max, float dist, float log_scale, int nlevels) {
  const float ratio = raw_max / dist;
  const float lg = (float)log((double)ratio);
  int ns = (int)ceilf(lg / log_scale);
  if (ns < 0) ns = 0; else if (ns >= nlevels) ns = nlevels - 1;
  return ns;
}

#endif
