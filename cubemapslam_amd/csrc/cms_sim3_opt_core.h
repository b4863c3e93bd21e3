// cms_sim3_opt_core.h -- the numeric core of Optimizer::OptimizeSim3 (src/Optimizer.cpp:888-1091): the two Sim3 edges
// (include/g2o_cubemap_vertices_edges.h:137-209), g2o::Sim3 (ThirdParty/g2o/g2o/types/sim3.h), VertexSim3Expmap::oplusImpl
// (types_seven_dof_expmap.h:60-69), g2o's numeric linearizeOplus (core/base_binary_edge.hpp:130-205), the robust quadratic form
// (base_binary_edge.hpp:55-120) and the Levenberg step (core/optimization_algorithm_levenberg.cpp:61-164).  ONE source for the host build
// (libcubemapslam_host.so: hm_sim3_optimize_host, the definition of record) and for the gfx950 kernel (cms_sim3_opt_kernels.hip).  This
// header compiles under g++ as it stands.
//
// Determinism contract (that of cms_sim3_core.h): plain IEEE + - * / sqrt in the order this source fixes, -ffp-contract=off on both builds, no
// fma(), no reciprocal builtins, no libm beyond sqrt / fabs.  exp, sin and cos are this header's own fixed-order polynomials (cms_det_exp,
// cms_det_sincos): libm's and the device library's differ from each other in the last place, and a Sim3 that differs in the last place
// flips float residuals.  The same inputs give the same bits from g++ and from hipcc.
//
//   edges      e12 = m1 - proj(face1, S.map(X2)), e21 = m2 - proj(face2, S.inverse().map(X1)); proj narrows the point to float and returns
//              float u, v (multipinhole_project, src/g2o_cubemap_vertices_edges.cpp:279-287, TransformRaysToTargetFace: no bounds test)
//   jacobian   CMS_SIM3_OPT_AS_WRITTEN: g2o's central differences with delta = 1e-9 on the Sim3 vertex -- both edges have linearizeOplus
//              commented out -- through the float-narrowed projection, so almost every entry is an exact 0 and the others are one float
//              ulp / 2e-9.  CMS_SIM3_OPT_ANALYTIC: the derivative of the double projection (header of cms_s3o_pair_jac).  Errors and chi2
//              go through the float-narrowed projection in both
//   sums       pair k's two edges (e12, then e21) add into slot k mod CMS_SIM3_OPT_SLOTS in ascending k; the slots are folded by
//              cms_s3o_tree.  The chi2 of a linearisation and of a trial come out of the same slots and the same tree, so a trial that changes
//              no float residual gives rho == 0 exactly and ends the round, as in g2o, where both sums are one function
//   solve      the unpivoted dense LDL^T of pose_solve6 (cms_pose_opt.hip) on 7 x 7; a zero or non-finite pivot is a failed solve, the
//              update is then zero and the trial is rejected
//   NaN bits   every double that leaves the core is stored as the one quiet NaN 0x7FF8000000000000 when it is a NaN
#ifndef CMS_SIM3_OPT_CORE_H
#define CMS_SIM3_OPT_CORE_H
#include <math.h>
#include <stdint.h>
#include "cms_detmath.h"      // CMS_HD

#define CMS_SIM3_OPT_AS_WRITTEN 0
#define CMS_SIM3_OPT_ANALYTIC 1
#define CMS_SIM3_OPT_SLOTS 256
#define CMS_SIM3_OPT_ACC 36         // [0..28) upper triangle of H row by row, [28..35) b, [35] chi2

CMS_HD double cms_s3o_canon(double v) { return v == v ? v : __builtin_nan(""); }

// ---- exp, sin, cos in double: Cody-Waite reduction, then the Taylor series in Horner form (remainder below 1e-18 of the value)
CMS_HD double cms_det_exp(double x) {
  if (!(x == x)) return __builtin_nan("");
  if (x > 709.0) return __builtin_inf();
  if (x < -708.0) return 0.0;
  const double kd = __builtin_rint(x * 1.44269504088896338700e+00);
  const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;      // ln 2 in two parts: k * hi is exact
  double p = 1.0 / 355687428096000.0;        // 1/17!   (|r| <= 0.3466: r^18 / 18! < 1e-24)
  p = p * r + 1.0 / 20922789888000.0;        // 1/16!
  p = p * r + 1.0 / 1307674368000.0;         // 1/15!
  p = p * r + 1.0 / 87178291200.0;           // 1/14!
  p = p * r + 1.0 / 6227020800.0;            // 1/13!
  p = p * r + 1.0 / 479001600.0;             // 1/12!
  p = p * r + 1.0 / 39916800.0;              // 1/11!
  p = p * r + 1.0 / 3628800.0;               // 1/10!
  p = p * r + 1.0 / 362880.0;                // 1/9!
  p = p * r + 1.0 / 40320.0;                 // 1/8!
  p = p * r + 1.0 / 5040.0;                  // 1/7!
  p = p * r + 1.0 / 720.0;                   // 1/6!
  p = p * r + 1.0 / 120.0;                   // 1/5!
  p = p * r + 1.0 / 24.0;                    // 1/4!
  p = p * r + 1.0 / 6.0;                     // 1/3!
  p = p * r + 0.5;
  const double e = 1.0 + (r + (r * r) * p);
  const unsigned long long bits = (unsigned long long)((int)kd + 1023) << 52;      // 2^k, -1021 <= k <= 1023
  double two_k;
  __builtin_memcpy(&two_k, &bits, 8);
  return e * two_k;
}

CMS_HD void cms_det_sincos(double x, double* s_out, double* c_out) {
  if (!(fabs(x) <= 1.0e5)) { *s_out = __builtin_nan(""); *c_out = __builtin_nan(""); return; }      // beyond the reduction's reach, or NaN
  const double kd = __builtin_rint(x * 0.63661977236758134308);
  // pi/2 in three parts (33 + 33 bits, then the rest): k * the first two is exact
  const double r = ((x - kd * 1.57079632673412561417e+00) - kd * 6.07710050630396597660e-11) - kd * 2.02226624879595063154e-21;
  const double r2 = r * r;
  double sp = 1.0 / 355687428096000.0;             // 1/17!   (|r| <= pi/4: r^19 / 19! < 1e-19)
  sp = sp * r2 - 1.0 / 1307674368000.0;            // 1/15!
  sp = sp * r2 + 1.0 / 6227020800.0;               // 1/13!
  sp = sp * r2 - 1.0 / 39916800.0;                 // 1/11!
  sp = sp * r2 + 1.0 / 362880.0;                   // 1/9!
  sp = sp * r2 - 1.0 / 5040.0;                     // 1/7!
  sp = sp * r2 + 1.0 / 120.0;                      // 1/5!
  sp = sp * r2 - 1.0 / 6.0;                        // 1/3!
  const double sn = r + r * (r2 * sp);
  double cp = -1.0 / 6402373705728000.0;           // 1/18!
  cp = cp * r2 + 1.0 / 20922789888000.0;           // 1/16!
  cp = cp * r2 - 1.0 / 87178291200.0;              // 1/14!
  cp = cp * r2 + 1.0 / 479001600.0;                // 1/12!
  cp = cp * r2 - 1.0 / 3628800.0;                  // 1/10!
  cp = cp * r2 + 1.0 / 40320.0;                    // 1/8!
  cp = cp * r2 - 1.0 / 720.0;                      // 1/6!
  cp = cp * r2 + 1.0 / 24.0;                       // 1/4!
  cp = cp * r2 - 0.5;
  const double cs = 1.0 + r2 * cp;
  const int q = ((int)kd) & 3;
  if (q == 0) { *s_out = sn; *c_out = cs; }
  else if (q == 1) { *s_out = cs; *c_out = -sn; }
  else if (q == 2) { *s_out = -sn; *c_out = -cs; }
  else { *s_out = -cs; *c_out = sn; }
}

// ---- g2o::Sim3: r (Eigen::Quaterniond, stored x y z w), t, s
struct CmsS3 { double q[4], t[3], s; };

// Eigen's Quaternion * Vector3: uv = vec x v; uv += uv; v + w * uv + vec x uv
CMS_HD void cms_s3o_rotate(const double* q, const double* v, double* o) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  double u0 = y * v[2] - z * v[1], u1 = z * v[0] - x * v[2], u2 = x * v[1] - y * v[0];
  u0 += u0; u1 += u1; u2 += u2;
  const double c0 = y * u2 - z * u1, c1 = z * u0 - x * u2, c2 = x * u1 - y * u0;
  const double o0 = (v[0] + w * u0) + c0, o1 = (v[1] + w * u1) + c1, o2 = (v[2] + w * u2) + c2;
  o[0] = o0; o[1] = o1; o[2] = o2;
}
CMS_HD void cms_s3o_quat_mul(const double* a, const double* b, double* o) {
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}
// Eigen::Quaterniond(Matrix3d), m row major
CMS_HD void cms_s3o_R_to_quat(const double* m, double* q) {
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t; t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    return;
  }
  int i = 0;
  if (m[4] > m[0]) i = 1;
  if (m[8] > (i ? m[4] : m[0])) i = 2;
  if (i == 0) {
    t = sqrt(m[0] - m[4] - m[8] + 1.0);
    q[0] = 0.5 * t; t = 0.5 / t;
    q[3] = (m[7] - m[5]) * t; q[1] = (m[3] + m[1]) * t; q[2] = (m[6] + m[2]) * t;
  } else if (i == 1) {
    t = sqrt(m[4] - m[8] - m[0] + 1.0);
    q[1] = 0.5 * t; t = 0.5 / t;
    q[3] = (m[2] - m[6]) * t; q[2] = (m[7] + m[5]) * t; q[0] = (m[1] + m[3]) * t;
  } else {
    t = sqrt(m[8] - m[0] - m[4] + 1.0);
    q[2] = 0.5 * t; t = 0.5 / t;
    q[3] = (m[3] - m[1]) * t; q[0] = (m[2] + m[6]) * t; q[1] = (m[5] + m[7]) * t;
  }
}
// Eigen's toRotationMatrix, row major
CMS_HD void cms_s3o_quat_to_R(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
// Sim3(const Matrix3d& R, const Vector3d& t, double s): gScm of src/LoopClosing.cpp:324
CMS_HD void cms_s3o_from_Rts(const double* R, const double* t, double s, CmsS3* o) {
  cms_s3o_R_to_quat(R, o->q);
  o->t[0] = t[0]; o->t[1] = t[1]; o->t[2] = t[2]; o->s = s;
}
CMS_HD void cms_s3o_map(const CmsS3& S, const double* X, double* y) {      // s * (r * xyz) + t
  double r[3];
  cms_s3o_rotate(S.q, X, r);
  y[0] = S.s * r[0] + S.t[0]; y[1] = S.s * r[1] + S.t[1]; y[2] = S.s * r[2] + S.t[2];
}
CMS_HD void cms_s3o_inverse(const CmsS3& S, CmsS3* o) {                     // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
  const double qc[4] = {-S.q[0], -S.q[1], -S.q[2], S.q[3]};
  const double k = -1. / S.s;
  const double v[3] = {k * S.t[0], k * S.t[1], k * S.t[2]};
  double t[3];
  cms_s3o_rotate(qc, v, t);
  o->q[0] = qc[0]; o->q[1] = qc[1]; o->q[2] = qc[2]; o->q[3] = qc[3];
  o->t[0] = t[0]; o->t[1] = t[1]; o->t[2] = t[2];
  o->s = 1. / S.s;
}
CMS_HD void cms_s3o_mul(const CmsS3& a, const CmsS3& b, CmsS3* o) {         // operator*: no renormalisation
  double q[4], r[3];
  cms_s3o_quat_mul(a.q, b.q, q);
  cms_s3o_rotate(a.q, b.t, r);
  const double t0 = a.s * r[0] + a.t[0], t1 = a.s * r[1] + a.t[1], t2 = a.s * r[2] + a.t[2];
  const double s = a.s * b.s;
  o->q[0] = q[0]; o->q[1] = q[1]; o->q[2] = q[2]; o->q[3] = q[3];
  o->t[0] = t0; o->t[1] = t1; o->t[2] = t2; o->s = s;
}
// Sim3(const Vector7d& update) (sim3.h:70-142): update = omega | upsilon | sigma
CMS_HD void cms_s3o_exp(const double* u, CmsS3* o) {
  const double om0 = u[0], om1 = u[1], om2 = u[2], sigma = u[6];
  const double theta = sqrt(om0 * om0 + om1 * om1 + om2 * om2);
  const double Om[9] = {0, -om2, om1, om2, 0, -om0, -om1, om0, 0};
  const double s = cms_det_exp(sigma);
  double Om2[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Om2[3 * i + j] = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
  const double eps = 0.00001;
  double A, B, C, R[9];
  bool small = theta < eps;
  double sn = 0, cs = 0;
  if (!small) cms_det_sincos(theta, &sn, &cs);
  if (fabs(sigma) < eps) {
    C = 1;
    if (small) {
      A = 1. / 2.; B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cs) / theta2;
      B = (theta - sn) / (theta2 * theta);
    }
  } else {
    C = (s - 1) / sigma;
    if (small) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      const double a = s * sn, b = s * cs, theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
  if (small) {
    for (int i = 0; i < 9; ++i) R[i] = (((i & 3) == 0 ? 1.0 : 0.0) + Om[i]) + Om2[i];
  } else {
    const double ka = sn / theta, kb = (1 - cs) / (theta * theta);
    for (int i = 0; i < 9; ++i) R[i] = (((i & 3) == 0 ? 1.0 : 0.0) + ka * Om[i]) + kb * Om2[i];
  }
  cms_s3o_R_to_quat(R, o->q);
  double W[9];
  for (int i = 0; i < 9; ++i) W[i] = (A * Om[i] + B * Om2[i]) + C * ((i & 3) == 0 ? 1.0 : 0.0);
  for (int i = 0; i < 3; ++i) o->t[i] = W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5];
  o->s = s;
}
// VertexSim3Expmap::oplusImpl: under _fix_scale the caller's update[6] is zeroed in place, then estimate <- Sim3(update) * estimate
CMS_HD void cms_s3o_oplus(const CmsS3& S, double* u, int fix_scale, CmsS3* o) {
  if (fix_scale) u[6] = 0;
  CmsS3 E;
  cms_s3o_exp(u, &E);
  cms_s3o_mul(E, S, o);
}

// ---- the camera: FaceInCubemap(cv::Point2f) (include/CamModelGeneral.h:445-456: float / int, widened), GetPosInFace<double> (:204-209) and
// TransformRaysToTargetFace (src/CamModelGeneral.cpp:228-263).  Faces: 0 front, 1 left, 2 right, 3 upper, 4 lower
CMS_HD int cms_s3o_face_in_cubemap(int F, float x, float y) {
  const double i = (double)(x / (float)F), j = (double)(y / (float)F);
  if (i >= 0 && i < 1 && j >= 1 && j < 2) return 1;
  if (i >= 1 && i < 2 && j >= 0 && j < 1) return 3;
  if (i >= 1 && i < 2 && j >= 1 && j < 2) return 0;
  if (i >= 1 && i < 2 && j >= 2 && j < 3) return 4;
  if (i >= 2 && i < 3 && j >= 1 && j < 2) return 2;
  return -1;
}
// u - floor(u / F) * F in double for a key point inside a face (0 <= u / F < 3: the truncation is the floor)
CMS_HD double cms_s3o_pos_in_face(int F, float uc) {
  const double u = (double)uc;
  const int i = (int)(u / F);
  return u - i * F;
}
CMS_HD void cms_s3o_face_local(int face, double x, double y, double z, double* l) {      // cvtRigToFaces
  switch (face) {
    case 0: l[0] = x; l[1] = y; l[2] = z; break;
    case 1: l[0] = z; l[1] = y; l[2] = -x; break;
    case 2: l[0] = -z; l[1] = y; l[2] = x; break;
    case 3: l[0] = x; l[1] = z; l[2] = -y; break;
    default: l[0] = x; l[1] = -z; l[2] = y; break;
  }
}
// multipinhole_project: the point narrowed to cv::Vec3f, `_x * fx / _z + cx` in double (fx = cx = F / 2 are double members), narrowed to float
CMS_HD void cms_s3o_project(int F, int face, const double* y, double* uv) {
  const double f = F / 2.0;
  double l[3];
  cms_s3o_face_local(face, (double)(float)y[0], (double)(float)y[1], (double)(float)y[2], l);
  uv[0] = (double)(float)(l[0] * f / l[2] + f);
  uv[1] = (double)(float)(l[1] * f / l[2] + f);
}

// ---- one kept correspondence as the graph holds it (:941-1028)
struct CmsS3oPair {
  double X1[3], X2[3];      // vPoint1 / vPoint2: P3D1c, P3D2c (float) widened; both fixed
  double m1[2], m2[2];      // _measurementInFace of e12 / e21
  double om1, om2;          // information = Identity * invSigma2 (float widened)
  int face1, face2;
};
// false: a key point lies in no face (the reference's computeError would exit())
CMS_HD bool cms_s3o_pair_setup(int F, const float* x1, const float* x2, const float* kp1, const float* kp2, float is1, float is2, CmsS3oPair* p) {
  for (int i = 0; i < 3; ++i) { p->X1[i] = (double)x1[i]; p->X2[i] = (double)x2[i]; }
  p->face1 = cms_s3o_face_in_cubemap(F, kp1[0], kp1[1]);
  p->face2 = cms_s3o_face_in_cubemap(F, kp2[0], kp2[1]);
  p->m1[0] = cms_s3o_pos_in_face(F, kp1[0]); p->m1[1] = cms_s3o_pos_in_face(F, kp1[1]);
  p->m2[0] = cms_s3o_pos_in_face(F, kp2[0]); p->m2[1] = cms_s3o_pos_in_face(F, kp2[1]);
  p->om1 = (double)is1; p->om2 = (double)is2;
  return p->face1 >= 0 && p->face2 >= 0;
}
// computeError of both edges: e[0..1] = e12, e[2..3] = e21
CMS_HD void cms_s3o_errors(int F, const CmsS3oPair& p, const CmsS3& S, const CmsS3& Sinv, double* e) {
  double y[3], uv[2];
  cms_s3o_map(S, p.X2, y);
  cms_s3o_project(F, p.face1, y, uv);
  e[0] = p.m1[0] - uv[0]; e[1] = p.m1[1] - uv[1];
  cms_s3o_map(Sinv, p.X1, y);
  cms_s3o_project(F, p.face2, y, uv);
  e[2] = p.m2[0] - uv[0]; e[3] = p.m2[1] - uv[1];
}
// BaseEdge::chi2(): _error.dot(information() * _error) with information = om * I
CMS_HD double cms_s3o_chi2(double om, const double* e) { return e[0] * (om * e[0]) + e[1] * (om * e[1]); }
// RobustKernelHuber::robustify: rho[0] returned, rho[1] in *w
CMS_HD double cms_s3o_huber(double e2, double delta, double* w) {
  const double dsqr = delta * delta;
  if (e2 <= dsqr) { *w = 1.0; return e2; }
  const double sq = sqrt(e2);
  *w = delta / sq;
  return 2 * sq * delta - dsqr;
}

// ---- what a linearisation needs of the estimate, shared by all pairs: the estimate and its inverse, and for the numeric Jacobian the
// fourteen perturbed estimates of linearizeOplus (P[2 d] = oplus(+delta e_d), P[2 d + 1] = oplus(-delta e_d)) with their inverses
struct CmsS3oLin {
  CmsS3 S, Sinv;
  CmsS3 P[14], Pinv[14];
  double R[9];            // S's rotation matrix (analytic mode)
};
CMS_HD void cms_s3o_lin_base(const CmsS3& S, CmsS3oLin* L) {
  L->S = S;
  cms_s3o_inverse(S, &L->Sinv);
  cms_s3o_quat_to_R(S.q, L->R);
}
CMS_HD void cms_s3o_lin_perturb(const CmsS3& S, int fix_scale, int k, CmsS3oLin* L) {      // k in [0, 14)
  double add[7] = {0, 0, 0, 0, 0, 0, 0};
  add[k >> 1] = (k & 1) ? -1e-9 : 1e-9;
  cms_s3o_oplus(S, add, fix_scale, &L->P[k]);
  cms_s3o_inverse(L->P[k], &L->Pinv[k]);
}

// The 2 x 3 derivative of the face projection in the camera frame at y (double, not narrowed): rows of G Rf, G = [f/lz 0 -f lx/lz^2; 0 f/lz -f ly/lz^2]
CMS_HD void cms_s3o_jpi(int F, int face, const double* y, double* Jc) {
  const double f = F / 2.0;
  double l[3];
  cms_s3o_face_local(face, y[0], y[1], y[2], l);
  const double g0 = f / l[2], g02 = -(f * l[0]) / (l[2] * l[2]), g12 = -(f * l[1]) / (l[2] * l[2]);
  // column j of Jc = sign * column k of G, where camera axis j is face axis k
  switch (face) {
    case 0: Jc[0] = g0; Jc[1] = 0; Jc[2] = g02; Jc[3] = 0; Jc[4] = g0; Jc[5] = g12; break;
    case 1: Jc[0] = -g02; Jc[1] = 0; Jc[2] = g0; Jc[3] = -g12; Jc[4] = g0; Jc[5] = 0; break;
    case 2: Jc[0] = g02; Jc[1] = 0; Jc[2] = -g0; Jc[3] = g12; Jc[4] = g0; Jc[5] = 0; break;
    case 3: Jc[0] = g0; Jc[1] = -g02; Jc[2] = 0; Jc[3] = 0; Jc[4] = -g12; Jc[5] = g0; break;
    default: Jc[0] = g0; Jc[1] = g02; Jc[2] = 0; Jc[3] = 0; Jc[4] = g12; Jc[5] = -g0; break;
  }
}
// J (2 x 7, row major) = sgn * M [ -[p]x | I | p ] for a 2 x 3 M
CMS_HD void cms_s3o_jac_rows(const double* M, const double* p, double sgn, double* J) {
  for (int i = 0; i < 2; ++i) {
    const double m0 = M[3 * i], m1 = M[3 * i + 1], m2 = M[3 * i + 2];
    J[7 * i] = sgn * (m2 * p[1] - m1 * p[2]);
    J[7 * i + 1] = sgn * (m0 * p[2] - m2 * p[0]);
    J[7 * i + 2] = sgn * (m1 * p[0] - m0 * p[1]);
    J[7 * i + 3] = sgn * m0; J[7 * i + 4] = sgn * m1; J[7 * i + 5] = sgn * m2;
    J[7 * i + 6] = sgn * ((m0 * p[0] + m1 * p[1]) + m2 * p[2]);
  }
}
// _jacobianOplusXj of both edges (2 x 7 each, row major) at L->S.
//   as written  column d = (1 / (2 * 1e-9)) * (e(oplus(+delta e_d)) - e(oplus(-delta e_d)))
//   analytic    for the update S <- exp(u) S: y = S X2, de12/du = -Jpi(y) [ -[y]x | I | y ];
//               y = S^-1 X1, de21/du = +Jpi(y) (1/s) R^T [ -[X1]x | I | X1 ];  under fix_scale column 6 is 0, as the as-written mode gives it
CMS_HD void cms_s3o_pair_jac(int F, int mode, int fix_scale, const CmsS3oPair& p, const CmsS3oLin& L, double* J12, double* J21) {
  if (mode == CMS_SIM3_OPT_AS_WRITTEN) {
    const double scalar = 1.0 / (2 * 1e-9);
    for (int d = 0; d < 7; ++d) {
      double ep[4], em[4];
      cms_s3o_errors(F, p, L.P[2 * d], L.Pinv[2 * d], ep);
      cms_s3o_errors(F, p, L.P[2 * d + 1], L.Pinv[2 * d + 1], em);
      J12[d] = scalar * (ep[0] - em[0]); J12[7 + d] = scalar * (ep[1] - em[1]);
      J21[d] = scalar * (ep[2] - em[2]); J21[7 + d] = scalar * (ep[3] - em[3]);
    }
    return;
  }
  double y[3], Jc[6];
  cms_s3o_map(L.S, p.X2, y);
  cms_s3o_jpi(F, p.face1, y, Jc);
  cms_s3o_jac_rows(Jc, y, -1.0, J12);
  cms_s3o_map(L.Sinv, p.X1, y);
  cms_s3o_jpi(F, p.face2, y, Jc);
  const double is = 1.0 / L.S.s;
  double M[6];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 3; ++j)      // (1/s) R^T: entry (k, j) = is * R[j][k]
      M[3 * i + j] = (Jc[3 * i] * (is * L.R[3 * j]) + Jc[3 * i + 1] * (is * L.R[3 * j + 1])) + Jc[3 * i + 2] * (is * L.R[3 * j + 2]);
  cms_s3o_jac_rows(M, p.X1, 1.0, J21);
  if (fix_scale) { J12[6] = 0; J12[13] = 0; J21[6] = 0; J21[13] = 0; }
}
// constructQuadraticForm of one edge with its Huber kernel into acc: H += B^T (rho1 om) B, b += B^T (rho1 * -(om e)), chi2 += rho0
CMS_HD void cms_s3o_edge_accumulate(const double* J, const double* e, double om, double delta, double* acc) {
  double w;
  const double rho0 = cms_s3o_huber(cms_s3o_chi2(om, e), delta, &w);
  const double ow = w * om;
  const double r0 = -(om * e[0]) * w, r1 = -(om * e[1]) * w;
  int k = 0;
  for (int i = 0; i < 7; ++i)
    for (int j = i; j < 7; ++j) acc[k++] += (J[i] * ow) * J[j] + (J[7 + i] * ow) * J[7 + j];
  for (int i = 0; i < 7; ++i) acc[28 + i] += J[i] * r0 + J[7 + i] * r1;
  acc[35] += rho0;
}
// activeRobustChi2's share of one pair, in the order of cms_s3o_edge_accumulate's chi2 (e12, then e21)
CMS_HD void cms_s3o_pair_chi(const CmsS3oPair& p, const double* e, double delta, double* chi) {
  double w;
  *chi += cms_s3o_huber(cms_s3o_chi2(p.om1, e), delta, &w);
  *chi += cms_s3o_huber(cms_s3o_chi2(p.om2, e + 2), delta, &w);
}

// The fold of the slots: inside every group of 64, s[i] += s[i + o] for o = 32, 16, ..., 1; then (g0 + g1) + (g2 + g3).  The kernel realises the
// first part as a wavefront's xor butterfly (the same additions: IEEE addition commutes) and the second through LDS.  `s` is destroyed.
CMS_HD double cms_s3o_tree(double* s) {
  for (int g = 0; g < CMS_SIM3_OPT_SLOTS; g += 64)
    for (int o = 32; o > 0; o >>= 1)
      for (int i = 0; i < o; ++i) s[g + i] = s[g + i] + s[g + i + o];
  return (s[0] + s[64]) + (s[128] + s[192]);
}

// dense LDL^T of (H + lambda I) x = b, 7 x 7; false on a zero / non-finite pivot
CMS_HD bool cms_s3o_solve7(const double* H, const double* b, double lambda, double* x) {
  double A[49], D[7], RD[7];
  for (int i = 0; i < 49; ++i) A[i] = H[i];
  for (int i = 0; i < 7; ++i) A[8 * i] += lambda;
  bool ok = true;
  for (int j = 0; j < 7; ++j) {
    double d = A[8 * j];
    for (int k = 0; k < j; ++k) d -= A[7 * j + k] * A[7 * j + k] * D[k];
    if (!(d - d == 0.0) || d == 0.0) ok = false;      // d - d is 0 exactly for a finite d
    D[j] = d;
    const double rd = 1.0 / d;
    RD[j] = rd;
    for (int i = j + 1; i < 7; ++i) {
      double s = A[7 * i + j];
      for (int k = 0; k < j; ++k) s -= A[7 * i + k] * A[7 * j + k] * D[k];
      A[7 * i + j] = s * rd;
    }
  }
  for (int i = 0; i < 7; ++i) x[i] = b[i];
  for (int i = 0; i < 7; ++i)
    for (int k = 0; k < i; ++k) x[i] -= A[7 * i + k] * x[k];
  for (int i = 0; i < 7; ++i) x[i] *= RD[i];
  for (int i = 6; i >= 0; --i)
    for (int k = i + 1; k < 7; ++k) x[i] -= A[7 * k + i] * x[k];
  return ok;
}

// ---- OptimizationAlgorithmLevenberg::solve, the part one lane owns.  A caller runs, per iteration `it` of an optimize() call:
//   sums of a linearisation pass at lm.S -> cms_s3o_lm_begin;  then do { cms_s3o_lm_trial; the chi2 of an error pass at lm.trial ->
//   cms_s3o_lm_judge } while it returns true;  then cms_s3o_lm_stop says whether optimize() ends here.
struct CmsS3oLM {
  CmsS3 S, trial;
  double H[49], b[7];
  double lambda, ni, currentChi, iniChi, rho, scale;
  int nBad, qmax, ok2, fix_scale;
};
CMS_HD void cms_s3o_lm_begin(CmsS3oLM* m, const double* sum, int it) {
  int k = 0;
  for (int i = 0; i < 7; ++i)
    for (int j = i; j < 7; ++j) { m->H[7 * i + j] = sum[k]; m->H[7 * j + i] = sum[k]; ++k; }
  for (int i = 0; i < 7; ++i) m->b[i] = sum[28 + i];
  m->currentChi = sum[35]; m->iniChi = sum[35];
  if (it == 0) {      // computeLambdaInit: tau = 1e-5
    double md = 0;
    for (int j = 0; j < 7; ++j) { const double a = fabs(m->H[8 * j]); md = a > md ? a : md; }
    m->lambda = 1e-5 * md; m->ni = 2; m->nBad = 0;
  }
  m->rho = 0; m->qmax = 0;
}
CMS_HD void cms_s3o_lm_trial(CmsS3oLM* m) {
  double x[7];
  m->ok2 = cms_s3o_solve7(m->H, m->b, m->lambda, x) ? 1 : 0;
  if (!m->ok2) for (int i = 0; i < 7; ++i) x[i] = 0;
  cms_s3o_oplus(m->S, x, m->fix_scale, &m->trial);      // zeroes x[6] under fix_scale, as g2o does in the solver's own vector
  double scale = 0;
  for (int j = 0; j < 7; ++j) scale += x[j] * (m->lambda * x[j] + m->b[j]);
  m->scale = scale;
}
// true: another trial (rho < 0 && qmax < 10)
CMS_HD bool cms_s3o_lm_judge(CmsS3oLM* m, double chi) {
  const double tempChi = m->ok2 ? chi : 1.7976931348623157e308;
  m->rho = (m->currentChi - tempChi) / (m->scale + 1e-3);
  if (m->rho > 0 && (tempChi - tempChi == 0.0)) {
    const double t21 = 2 * m->rho - 1;
    double alpha = 1. - t21 * t21 * t21;      // pow(2 rho - 1, 3) as the cube, like cms_pose_opt.hip
    alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
    m->lambda *= (1. / 3. > alpha ? 1. / 3. : alpha);
    m->ni = 2; m->currentChi = tempChi;
    m->S = m->trial;
  } else {
    m->lambda *= m->ni; m->ni *= 2;
  }
  ++m->qmax;
  return m->rho < 0 && m->qmax < 10;
}
CMS_HD bool cms_s3o_lm_stop(CmsS3oLM* m) {
  if (m->qmax == 10 || m->rho == 0) return true;
  if ((m->iniChi - m->currentChi) * 1e3 < m->iniChi) ++m->nBad; else m->nBad = 0;
  return m->nBad >= 3;
}

// :1043 / :1077 on a pair's stored errors: true = the pair goes (th2 is the float argument, widened)
CMS_HD bool cms_s3o_pair_is_bad(const CmsS3oPair& p, const double* e, float th2) {
  return cms_s3o_chi2(p.om1, e) > (double)th2 || cms_s3o_chi2(p.om2, e + 2) > (double)th2;
}
// deltaHuber: `const float deltaHuber = sqrt(th2)` handed to setDelta(double)
CMS_HD double cms_s3o_huber_delta(float th2) { return (double)(float)sqrt((double)th2); }
// nMoreIterations (:1055-1059)
CMS_HD int cms_s3o_more_iterations(int nBad) { return nBad > 0 ? 10 : 5; }

#endif
