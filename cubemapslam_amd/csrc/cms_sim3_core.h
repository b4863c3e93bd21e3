// cms_sim3_core.h -- the numeric core of Sim3Solver (src/Sim3Solver.cpp:239-394): Horn's closed-form absolute orientation on three point pairs and
// the two-way inlier test, ONE source for the host build (libcubemapslam_host.so: hm_sim3_iterate_host, the definition of record) and for the
// gfx950 kernels (cms_sim3_kernels.hip).  This header compiles under g++ as it stands (tests/emu/sim3_core_emu.cpp includes it).
//
// Determinism contract: plain IEEE + - * / sqrt, float where the reference holds CV_32F and double where it computes in double, in the order
// this source fixes; both builds use -ffp-contract=off.  No fma(), no reciprocal / rsqrt builtins, no libm beyond sqrt / fabs, no allocation.
// The same inputs give the same bits from g++ and from hipcc.
//
// Choices where the reference calls OpenCV (DESIGN.md "Sim3Solver"):
//   products   a float matrix product (M = Pr2 Pr1^T, P3 = R Pr2, R X + t, -sRinv t) sums double(a) * double(b) upwards over the inner index
//              in double, adds the float addend in double last and narrows once -- what OpenCV's gemm does for small CV_32F operands
//   centroid   float sums (p0 + p1) + p2, then / 3.0f (cv::reduce CV_32F -> CV_32F, C / P.cols)
//   eigen      cv::eigen is replaced by a cyclic two-sided Jacobi in double on the float-stored N: pair order (0,1) (0,2) (0,3) (1,2) (1,3)
//              (2,3), at most CMS_SIM3_SWEEPS sweeps, a sweep starts only while the off-diagonal square sum is > (DBL_EPSILON * diagonal
//              square sum's root)^2 -- false for NaN, so NaN ends it.  The largest eigenvalue is chosen "first maximum wins"; its vector is narrowed to float
//              (evec is CV_32F in the reference)
//   rotation   atan2 -> angle-axis -> cv::Rodrigues is the rotation of the unit quaternion (w, x, y, z) = evec / |evec|: R is built from the
//              quaternion's products in double, divided by w^2 + x^2 + y^2 + z^2, narrowed per element.  No transcendental, no sqrt.  One stated
//              difference: for an exactly zero imaginary part the reference divides 0 / 0 (NaN pose); this gives the identity
//   scale      nom = sum of double(Pr1) * double(P3), den = sum of the float squares P3 * P3 widened, both row major; ms12i = (float)(nom / den)
// Degenerate inputs: coincident points give M = 0, R = I, den = 0, s = NaN (when the float centroid of three equal points is the point itself;
// otherwise a rounding residue takes M's place); NaN / inf flow through and every comparison with them is false.  Nothing traps, nothing loops.
//   NaN bits   IEEE leaves sign and payload of a NaN an invalid operation makes to the implementation (x86 makes 0xFFC00000, gfx950 0x7FC00000), so
//              every float of the motion that is a NaN is stored as the one quiet NaN 0x7FC00000: what leaves the core has the same bits on both
#ifndef CMS_SIM3_CORE_H
#define CMS_SIM3_CORE_H
#include <float.h>
#include <math.h>
#include "cms_cubemap_project.h"      // CMS_HD, track_rays_to_cubemap = CamModelGeneral::TransformRaysToCubemap
#include "cms_ransac_core.h"          // cms_ransac_resolve_draws: the draws of one iteration

#define CMS_SIM3_SWEEPS 16

// What compute_sim3 leaves behind for a caller that wants to see the stages (the CPU tests); the kernels pass NULL.
struct CmsSim3Stages {
  float O1[3], O2[3], Pr1[9], Pr2[9];      // centroids; relative coordinates, 3 x 3 with one point per COLUMN as in the reference
  float M[9], N[16];
  double evals[4], evecs[16];              // Jacobi: eigenvalues (the diagonal, unsorted) and eigenvectors as COLUMNS
  int sweeps, chosen;
  float q[4];                              // the chosen eigenvector (w, x, y, z), not normalised
  float P3[9];
  double nom, den;
};

// The motion one hypothesis gives: mR12i, mt12i, ms12i, mT12i and mT21i (rows 0..2 of the 4 x 4, row major)
struct CmsSim3Motion {
  float R[9], t[3], s, T12[12], T21[12];
};

// Eigen decomposition of a symmetric 4 x 4 (A row major, destroyed: its diagonal becomes the eigenvalues), V's columns the eigenvectors.
// Returns the number of sweeps done.
CMS_HD int cms_sim3_jacobi4(double* A, double* V) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) V[4 * i + j] = i == j ? 1.0 : 0.0;
  int sweep = 0;
  for (; sweep < CMS_SIM3_SWEEPS; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int p = 0; p < 4; ++p) {
      diag += A[5 * p] * A[5 * p];
      for (int q = p + 1; q < 4; ++q) off += A[4 * p + q] * A[4 * p + q];
    }
    if (!(off > DBL_EPSILON * DBL_EPSILON * diag)) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[4 * p + q];
        if (apq == 0.0) continue;
        const double theta = (A[5 * q] - A[5 * p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 4; ++k) {      // A <- A J
          const double akp = A[4 * k + p], akq = A[4 * k + q];
          A[4 * k + p] = c * akp - s * akq;
          A[4 * k + q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {      // A <- J^T A
          const double apk = A[4 * p + k], aqk = A[4 * q + k];
          A[4 * p + k] = c * apk - s * aqk;
          A[4 * q + k] = s * apk + c * aqk;
        }
        A[4 * p + q] = 0.0; A[4 * q + p] = 0.0;
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[4 * k + p], vkq = V[4 * k + q];
          V[4 * k + p] = c * vkp - s * vkq;
          V[4 * k + q] = s * vkp + c * vkq;
        }
      }
  }
  return sweep;
}

// R of the quaternion (w, x, y, z) / |.|, row major
CMS_HD void cms_sim3_quat_to_R(const float* qf, float* R) {
  const double w = qf[0], x = qf[1], y = qf[2], z = qf[3];
  const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
  const double n2 = ww + xx + yy + zz;
  const double xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  R[0] = (float)((ww + xx - yy - zz) / n2); R[1] = (float)(2.0 * (xy - wz) / n2);     R[2] = (float)(2.0 * (xz + wy) / n2);
  R[3] = (float)(2.0 * (xy + wz) / n2);     R[4] = (float)((ww - xx + yy - zz) / n2); R[5] = (float)(2.0 * (yz - wx) / n2);
  R[6] = (float)(2.0 * (xz - wy) / n2);     R[7] = (float)(2.0 * (yz + wx) / n2);     R[8] = (float)((ww - xx - yy + zz) / n2);
}

CMS_HD float cms_sim3_canon(float v) { return v == v ? v : __builtin_nanf(""); }

// (float)(A[row] . x + add): the gemm rule of the header comment; A's row is a0 a1 a2
CMS_HD float cms_sim3_row(const float* a, float x0, float x1, float x2, float add) {
  return (float)((double)a[0] * (double)x0 + (double)a[1] * (double)x1 + (double)a[2] * (double)x2 + (double)add);
}

// ComputeSim3 (:250-361) on three pairs: P1, P2 are 3 points x 3 coordinates (point k at P[3k..3k+2]).
CMS_HD void cms_sim3_compute(const float* P1, const float* P2, int fix_scale, CmsSim3Motion* m, CmsSim3Stages* st) {
  // Step 1: centroids and relative coordinates; Pr[3 * r + c] = coordinate r of point c
  float O1[3], O2[3], Pr1[9], Pr2[9];
  for (int r = 0; r < 3; ++r) {
    O1[r] = ((P1[r] + P1[3 + r]) + P1[6 + r]) / 3.0f;
    O2[r] = ((P2[r] + P2[3 + r]) + P2[6 + r]) / 3.0f;
    for (int c = 0; c < 3; ++c) { Pr1[3 * r + c] = P1[3 * c + r] - O1[r]; Pr2[3 * r + c] = P2[3 * c + r] - O2[r]; }
  }
  // Step 2: M = Pr2 * Pr1^T
  float M[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      M[3 * i + j] = (float)((double)Pr2[3 * i] * (double)Pr1[3 * j] + (double)Pr2[3 * i + 1] * (double)Pr1[3 * j + 1] + (double)Pr2[3 * i + 2] * (double)Pr1[3 * j + 2]);
  // Step 3: N, its ten entries in double from float M, stored as float
  const double N11 = (double)M[0] + (double)M[4] + (double)M[8];
  const double N12 = (double)M[5] - (double)M[7];
  const double N13 = (double)M[6] - (double)M[2];
  const double N14 = (double)M[1] - (double)M[3];
  const double N22 = (double)M[0] - (double)M[4] - (double)M[8];
  const double N23 = (double)M[1] + (double)M[3];
  const double N24 = (double)M[6] + (double)M[2];
  const double N33 = -(double)M[0] + (double)M[4] - (double)M[8];
  const double N34 = (double)M[5] + (double)M[7];
  const double N44 = -(double)M[0] - (double)M[4] + (double)M[8];
  const float Nf[16] = {(float)N11, (float)N12, (float)N13, (float)N14, (float)N12, (float)N22, (float)N23, (float)N24,
                        (float)N13, (float)N23, (float)N33, (float)N34, (float)N14, (float)N24, (float)N34, (float)N44};
  // Step 4: eigenvector of the highest eigenvalue
  double A[16], V[16];
  for (int k = 0; k < 16; ++k) A[k] = (double)Nf[k];
  const int sweeps = cms_sim3_jacobi4(A, V);
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (A[5 * k] > A[5 * best]) best = k;
  float q[4];
  for (int k = 0; k < 4; ++k) q[k] = (float)V[4 * k + best];
  cms_sim3_quat_to_R(q, m->R);
  // Step 5: rotate set 2
  float P3[9];
  for (int i = 0; i < 3; ++i)
    for (int c = 0; c < 3; ++c) P3[3 * i + c] = cms_sim3_row(m->R + 3 * i, Pr2[c], Pr2[3 + c], Pr2[6 + c], 0.0f);
  // Step 6: scale
  double nom = 0.0, den = 0.0;
  if (!fix_scale) {
    for (int k = 0; k < 9; ++k) nom += (double)Pr1[k] * (double)P3[k];
    for (int k = 0; k < 9; ++k) { const float sq = P3[k] * P3[k]; den += (double)sq; }
    m->s = (float)(nom / den);
  } else {
    m->s = 1.0f;
  }
  // Step 7: t = O1 - s R O2 (gemm with alpha = s, then the float difference)
  for (int i = 0; i < 3; ++i) {
    const double ro = (double)m->R[3 * i] * (double)O2[0] + (double)m->R[3 * i + 1] * (double)O2[1] + (double)m->R[3 * i + 2] * (double)O2[2];
    m->t[i] = O1[i] - (float)((double)m->s * ro);
  }
  // Step 8: T12 = [sR | t], T21 = [(1/s) R^T | -(1/s) R^T t]
  const double inv_s = 1.0 / (double)m->s;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      m->T12[4 * i + j] = m->s * m->R[3 * i + j];
      m->T21[4 * i + j] = (float)(inv_s * (double)m->R[3 * j + i]);
    }
    m->T12[4 * i + 3] = m->t[i];
  }
  for (int i = 0; i < 3; ++i)
    m->T21[4 * i + 3] = (float)(-((double)m->T21[4 * i] * (double)m->t[0] + (double)m->T21[4 * i + 1] * (double)m->t[1] + (double)m->T21[4 * i + 2] * (double)m->t[2]));
  for (int k = 0; k < 9; ++k) m->R[k] = cms_sim3_canon(m->R[k]);
  for (int k = 0; k < 3; ++k) m->t[k] = cms_sim3_canon(m->t[k]);
  m->s = cms_sim3_canon(m->s);
  for (int k = 0; k < 12; ++k) { m->T12[k] = cms_sim3_canon(m->T12[k]); m->T21[k] = cms_sim3_canon(m->T21[k]); }
  if (st) {
    for (int k = 0; k < 3; ++k) { st->O1[k] = O1[k]; st->O2[k] = O2[k]; }
    for (int k = 0; k < 9; ++k) { st->Pr1[k] = Pr1[k]; st->Pr2[k] = Pr2[k]; st->M[k] = M[k]; st->P3[k] = P3[k]; }
    for (int k = 0; k < 16; ++k) { st->N[k] = Nf[k]; st->evecs[k] = V[k]; }
    for (int k = 0; k < 4; ++k) { st->evals[k] = A[5 * k]; st->q[k] = q[k]; }
    st->sweeps = sweeps; st->chosen = best; st->nom = nom; st->den = den;
  }
}

// Project (:412-433) for one point: T's rows 0..2 (row major, 4 wide), then TransformRaysToCubemap; u, v are whatever it left
CMS_HD void cms_sim3_project(int F, const float* T, const float* X, float& u, float& v) {
  const float x = cms_sim3_row(T, X[0], X[1], X[2], T[3]);
  const float y = cms_sim3_row(T + 4, X[0], X[1], X[2], T[7]);
  const float z = cms_sim3_row(T + 8, X[0], X[1], X[2], T[11]);
  track_rays_to_cubemap(F, x, y, z, u, v);
}

// CheckInliers (:364-394) for one correspondence: X2 through T12 against P1im1 = the projection of X1, X1 through T21 against P2im2.  The
// unknown-face branch of :375-378 is dead (the if / else below it overwrites the flag), so the result is err1 < maxErr1 && err2 < maxErr2 on
// floats; dist.dot(dist) sums in double and narrows on assignment to the float err
CMS_HD bool cms_sim3_is_inlier(int F, const float* T12, const float* T21, const float* X1, const float* X2, float max_err1, float max_err2) {
  float p1u, p1v, p2u, p2v, au, av, bu, bv;
  track_rays_to_cubemap(F, X1[0], X1[1], X1[2], p1u, p1v);      // mvP1im1 (FromCameraToImage, :435-453)
  track_rays_to_cubemap(F, X2[0], X2[1], X2[2], p2u, p2v);      // mvP2im2
  cms_sim3_project(F, T12, X2, au, av);                         // vP2im1
  cms_sim3_project(F, T21, X1, bu, bv);                         // vP1im2
  const float d1x = p1u - au, d1y = p1v - av, d2x = bu - p2u, d2y = bv - p2v;
  const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
  const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
  return err1 < max_err1 && err2 < max_err2;
}

// The three draws of one iteration by the reference's swap-and-pop (cms_ransac_core.h)
CMS_HD void cms_sim3_resolve_draws(int N, const int* draws, int* idx) { cms_ransac_resolve_draws<3>(N, draws, idx); }

#endif
