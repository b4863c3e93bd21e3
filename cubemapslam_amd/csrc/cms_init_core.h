// cms_init_core.h -- the numeric core of Initializer::InitializeWithRays (src/Initializer.cpp:53-521): ComputeE21, CheckEssiential, DecomposeE,
// Triangulate, CheckRT and ReconstructE's decision, with CamModelGeneral::GetVectorSigma (src/CamModelGeneral.cpp:307-333).  ONE source for the host
// build (libcubemapslam_host.so: hm_init_two_view_host, the definition of record) and for the gfx950 kernels (cms_init_kernels.hip).  It compiles
// under g++ as it stands (tests/emu/init_core_emu.cpp includes it).
//
// Determinism contract: plain IEEE + - * / sqrt and comparisons, float where the reference computes in float (everything is CV_32F) and double
// where cv::Mat does, in the order this source fixes; both builds use -ffp-contract=off.  No fma, no hypot, no acos, no libm beyond sqrt / fabs in
// anything the device executes, no allocation: every array arrives as a pointer (the kernels hand over LDS for the 8 x 9 system).  The same inputs
// give the same bits from g++ and from hipcc.  The conventions are those of DESIGN.md section 2 and of cms_tri_kernels.hip's header: cv::norm and
// Mat::dot accumulate in double, Matx / Vec dot products are float, `a*(rowB+rowC) - s*rowD` is two addWeighted passes, Mat / scalar multiplies by
// (float)(1.0/(double)s), small gemm products are summed left to right, comparisons against double literals are made in double.
//
// The SVD is cv::JacobiSVDImpl_<float> as cms_tri_kernels.hip restates it (one-sided Hestenes Jacobi on the columns,
// double dot products, float rotations, at most 30 sweeps, descending selection sort, first maximum), with gamma = sqrt(p*p + beta*beta) in place
// of hypot.  ComputeE21's `vt.row(8)` of a FULL_UV SVD of the 8 x 9 matrix is, in OpenCV, the ninth vector of a completed basis and cannot be
// pinned; here it is the null vector the Jacobi on the NINE columns leaves: the column whose norm went to (nearly) zero, last after the sort.
// E therefore differs from the reference's by rounding and possibly by sign; CheckEssiential is quadratic in E and DecomposeE tries +-t.
//
// Non-finite inputs flow through: a NaN makes every comparison false as in the reference, the sweeps are bounded, nothing traps.
#ifndef CMS_INIT_CORE_H
#define CMS_INIT_CORE_H
#include <float.h>
#include <math.h>
#include "cms_cubemap_project.h"      // CMS_HD, track_rays_to_cubemap = CamModelGeneral::TransformRaysToCubemap
#include "cms_ransac_core.h"          // cms_ransac_resolve_draws: the draws of one iteration

#if defined(__HIPCC__)
#define CMS_INIT_UNROLL _Pragma("unroll")
#else
#define CMS_INIT_UNROLL
#endif

// What compute_e21 leaves behind for a caller that wants to see the stages (the CPU tests); the kernels pass NULL.
struct CmsInitStages {
  float A[72];            // the 8 x 9 matrix, row major, before the SVD
  float Vt[81];           // its right singular vectors (rows), descending
  double W[9];            // its singular values
  float Epre[9], w3[3], u3[9], vt3[9];
};

CMS_HD bool cms_init_finite(float x) { return fabsf(x) <= FLT_MAX; }

// Givens rotation of one Jacobi step from the two squared column norms and the columns' dot product.  JacobiSVDImpl_ computes s first and c from
// it when beta < 0, c first and s from it otherwise; written with selects so that the device holds c and s in registers.
CMS_HD void cms_init_rotation(double a, double b, double p, float& c, float& s) {
  p *= 2.0;
  const double beta = a - b, gamma = sqrt(p * p + beta * beta);
  const bool neg = beta < 0;
  const double arg = neg ? ((gamma - beta) * 0.5) / gamma : (gamma + beta) / (gamma * 2.0);
  const float first = (float)sqrt(arg);
  const float second = (float)(p / (gamma * (double)first * 2.0));
  c = neg ? second : first;
  s = neg ? first : second;
}

// The Jacobi on arrays in memory (the 8 x 9 system: LDS on the device).  In: At, n rows of length m = the columns of A.  Out: row k of At = A v_k,
// row k of Vt (n x n) = v_k, W descending.
CMS_HD void cms_init_jacobi_mem(int m, int n, float* At, float* Vt, double* W) {
  const float eps = FLT_EPSILON * 2;
  for (int i = 0; i < n; ++i) {
    double sd = 0;
    for (int k = 0; k < m; ++k) sd += (double)At[i * m + k] * (double)At[i * m + k];
    W[i] = sd;
    for (int k = 0; k < n; ++k) Vt[i * n + k] = i == k ? 1.0f : 0.0f;
  }
  for (int iter = 0; iter < 30; ++iter) {
    bool changed = false;
    for (int i = 0; i < n - 1; ++i)
      for (int j = i + 1; j < n; ++j) {
        float* Ai = At + i * m;
        float* Aj = At + j * m;
        double a = W[i], p = 0, b = W[j];
        for (int k = 0; k < m; ++k) p += (double)Ai[k] * (double)Aj[k];
        if (fabs(p) <= (double)eps * sqrt(a * b)) continue;
        float c, s;
        cms_init_rotation(a, b, p, c, s);
        a = 0; b = 0;
        for (int k = 0; k < m; ++k) {
          const float ai = Ai[k], aj = Aj[k];
          const float t0 = c * ai + s * aj;
          const float t1 = -s * ai + c * aj;
          Ai[k] = t0; Aj[k] = t1;
          a += (double)t0 * (double)t0; b += (double)t1 * (double)t1;
        }
        W[i] = a; W[j] = b;
        changed = true;
        float* Vi = Vt + i * n;
        float* Vj = Vt + j * n;
        for (int k = 0; k < n; ++k) {
          const float vi = Vi[k], vj = Vj[k];
          Vi[k] = c * vi + s * vj;
          Vj[k] = -s * vi + c * vj;
        }
      }
    if (!changed) break;
  }
  for (int i = 0; i < n; ++i) {
    double sd = 0;
    for (int k = 0; k < m; ++k) sd += (double)At[i * m + k] * (double)At[i * m + k];
    W[i] = sqrt(sd);
  }
  for (int i = 0; i < n - 1; ++i) {
    int j = i;
    for (int k = i + 1; k < n; ++k)
      if (W[j] < W[k]) j = k;
    if (i != j) {
      const double tw = W[i]; W[i] = W[j]; W[j] = tw;
      for (int k = 0; k < m; ++k) { const float tv = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = tv; }
      for (int k = 0; k < n; ++k) { const float tv = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = tv; }
    }
  }
}

// The same Jacobi for a square N x N system (3 x 3, 4 x 4) held in the caller's local arrays: every index is static once the loops are unrolled,
// so the device keeps the arrays in registers
template <int N>
CMS_HD void cms_init_jacobi_reg(float* At, float* Vt, double* W) {
  const float eps = FLT_EPSILON * 2;
  CMS_INIT_UNROLL
  for (int i = 0; i < N; ++i) {
    double sd = 0;
    CMS_INIT_UNROLL
    for (int k = 0; k < N; ++k) { sd += (double)At[N * i + k] * (double)At[N * i + k]; Vt[N * i + k] = i == k ? 1.0f : 0.0f; }
    W[i] = sd;
  }
  for (int iter = 0; iter < 30; ++iter) {
    bool changed = false;
    CMS_INIT_UNROLL
    for (int i = 0; i < N - 1; ++i)
      CMS_INIT_UNROLL
      for (int j = i + 1; j < N; ++j) {
        double a = W[i], p = 0, b = W[j];
        CMS_INIT_UNROLL
        for (int k = 0; k < N; ++k) p += (double)At[N * i + k] * (double)At[N * j + k];
        if (!(fabs(p) <= (double)eps * sqrt(a * b))) {
          float c, s;
          cms_init_rotation(a, b, p, c, s);
          a = 0; b = 0;
          CMS_INIT_UNROLL
          for (int k = 0; k < N; ++k) {
            const float ai = At[N * i + k], aj = At[N * j + k];
            const float t0 = c * ai + s * aj;
            const float t1 = -s * ai + c * aj;
            At[N * i + k] = t0; At[N * j + k] = t1;
            a += (double)t0 * (double)t0; b += (double)t1 * (double)t1;
          }
          W[i] = a; W[j] = b;
          changed = true;
          CMS_INIT_UNROLL
          for (int k = 0; k < N; ++k) {
            const float vi = Vt[N * i + k], vj = Vt[N * j + k];
            Vt[N * i + k] = c * vi + s * vj;
            Vt[N * j + k] = -s * vi + c * vj;
          }
        }
      }
    if (!changed) break;
  }
  CMS_INIT_UNROLL
  for (int i = 0; i < N; ++i) {
    double sd = 0;
    CMS_INIT_UNROLL
    for (int k = 0; k < N; ++k) sd += (double)At[N * i + k] * (double)At[N * i + k];
    W[i] = sqrt(sd);
  }
  // selection sort, descending, first maximum wins (the running maximum is compared instead of indexing W[j] dynamically)
  CMS_INIT_UNROLL
  for (int i = 0; i < N - 1; ++i) {
    int j = i;
    double wmax = W[i];
    CMS_INIT_UNROLL
    for (int k = i + 1; k < N; ++k)
      if (wmax < W[k]) { wmax = W[k]; j = k; }
    CMS_INIT_UNROLL
    for (int k = i + 1; k < N; ++k)
      if (j == k) {
        const double tw = W[i]; W[i] = W[k]; W[k] = tw;
        CMS_INIT_UNROLL
        for (int q = 0; q < N; ++q) {
          const float ta = At[N * i + q]; At[N * i + q] = At[N * k + q]; At[N * k + q] = ta;
          const float tv = Vt[N * i + q]; Vt[N * i + q] = Vt[N * k + q]; Vt[N * k + q] = tv;
        }
      }
  }
}

// C = A * B, 3 x 3 row major: cv::gemm's small path, float products summed left to right
CMS_HD void cms_init_gemm3(const float* A, const float* B, float* C) {
  CMS_INIT_UNROLL
  for (int i = 0; i < 3; ++i)
    CMS_INIT_UNROLL
    for (int j = 0; j < 3; ++j) {
      float t = A[3 * i] * B[j];
      t = t + A[3 * i + 1] * B[3 + j];
      t = t + A[3 * i + 2] * B[6 + j];
      C[3 * i + j] = t;
    }
}
CMS_HD double cms_init_ddot3(const float* a, const float* b) {
  double s = (double)a[0] * (double)b[0];
  s = s + (double)a[1] * (double)b[1];
  return s + (double)a[2] * (double)b[2];
}
CMS_HD double cms_init_dnorm3(const float* a) { return sqrt(cms_init_ddot3(a, a)); }

// cv::SVD::compute(A, w, u, vt) of a 3 x 3 float matrix: u(i,k) = (A v_k)(i) * (float)(1 / w_k), vt row k = v_k.  A direction without a singular
// value (w_k <= FLT_MIN: OpenCV fills it from a pseudo-random vector) is zero, and the third one is the cross product of the other two.
CMS_HD void cms_init_svd3(const float* A, float* w, float* u, float* vt) {
  float At[9];
  double W[3];
  CMS_INIT_UNROLL
  for (int i = 0; i < 3; ++i)
    CMS_INIT_UNROLL
    for (int k = 0; k < 3; ++k) At[3 * i + k] = A[3 * k + i];
  cms_init_jacobi_reg<3>(At, vt, W);
  CMS_INIT_UNROLL
  for (int k = 0; k < 3; ++k) {
    w[k] = (float)W[k];
    const float s = W[k] > (double)FLT_MIN ? (float)(1.0 / W[k]) : 0.0f;
    CMS_INIT_UNROLL
    for (int i = 0; i < 3; ++i) u[3 * i + k] = At[3 * k + i] * s;
  }
  if (W[1] > (double)FLT_MIN && !(W[2] > (double)FLT_MIN)) {
    u[2] = u[3] * u[7] - u[6] * u[4];
    u[5] = u[6] * u[1] - u[0] * u[7];
    u[8] = u[0] * u[4] - u[3] * u[1];
  }
}

// ComputeE21 (:158-195), row j of the 8 x 9 matrix from one ray pair, stored as column entries: At is 9 rows of length 8
CMS_HD void cms_init_fill_row(int j, const float* ray1, const float* ray2, float* At) {
  const float x1 = ray1[0], y1 = ray1[1], z1 = ray1[2];
  const float x2 = ray2[0], y2 = ray2[1], z2 = ray2[2];
  At[0 * 8 + j] = x2 * x1;
  At[1 * 8 + j] = x2 * y1;
  At[2 * 8 + j] = x2 * z1;
  At[3 * 8 + j] = y2 * x1;
  At[4 * 8 + j] = y2 * y1;
  At[5 * 8 + j] = y2 * z1;
  At[6 * 8 + j] = z2 * x1;
  At[7 * 8 + j] = z2 * y1;
  At[8 * 8 + j] = z2 * z1;
}
// ... and the rest of it: At 72 floats (filled), Vt 81 floats and W 9 doubles are the caller's; E 3 x 3 row major
CMS_HD void cms_init_e21_from_rows(float* At, float* Vt, double* W, float* E, CmsInitStages* st) {
  if (st)
    for (int i = 0; i < 8; ++i)
      for (int c = 0; c < 9; ++c) st->A[9 * i + c] = At[8 * c + i];
  cms_init_jacobi_mem(8, 9, At, Vt, W);
  float Epre[9], w[3], u[9], vt[9], D[9], UD[9];
  CMS_INIT_UNROLL
  for (int k = 0; k < 9; ++k) Epre[k] = Vt[72 + k];
  cms_init_svd3(Epre, w, u, vt);
  w[2] = 0;
  CMS_INIT_UNROLL
  for (int k = 0; k < 9; ++k) D[k] = 0.0f;
  D[0] = w[0]; D[4] = w[1]; D[8] = w[2];
  cms_init_gemm3(u, D, UD);
  cms_init_gemm3(UD, vt, E);
  if (st) {
    for (int k = 0; k < 81; ++k) st->Vt[k] = Vt[k];
    for (int k = 0; k < 9; ++k) { st->W[k] = W[k]; st->Epre[k] = Epre[k]; st->u3[k] = u[k]; st->vt3[k] = vt[k]; }
    for (int k = 0; k < 3; ++k) st->w3[k] = w[k];
  }
}

// FaceInCubemap(const cv::Point2f&): float / int, widened (include/CamModelGeneral.h:445-470).  0 front, 1 left, 2 right, 3 upper, 4 lower
CMS_HD int cms_init_face_in_cubemap(int F, float x, float y) {
  const double i = (double)(x / (float)F), j = (double)(y / (float)F);
  if (i >= 0 && i < 1 && j >= 1 && j < 2) return 1;
  if (i >= 1 && i < 2 && j >= 0 && j < 1) return 3;
  if (i >= 1 && i < 2 && j >= 1 && j < 2) return 0;
  if (i >= 1 && i < 2 && j >= 2 && j < 3) return 4;
  if (i >= 2 && i < 3 && j >= 1 && j < 2) return 2;
  return -1;
}
// floor(v / F) for GetPosInFace without floor(): exact for every quotient inside the image; 0 outside [-4, 4) (such a point is on no face,
// and GetVectorSigma is then 0/0 whatever the cell)
CMS_HD int cms_init_cell(float v, int F) {
  const float q = v / (float)F;
  if (!(q > -4.0f && q < 4.0f)) return 0;
  int i = (int)q;
  if ((float)i > q) --i;
  return i;
}
// CamModelGeneral::GetVectorSigma(key, normalRig, sigmaInPixel = 1) (CamModelGeneral.cpp:307-333): fx, cx, cy are the double F / 2
CMS_HD float cms_init_vector_sigma(int F, float kx, float ky, float na, float nb, float nc_) {
  const double fx = F / 2.0;
  float n0, n1;
  switch (cms_init_face_in_cubemap(F, kx, ky)) {       // cvtRigToFaces: only the local x, y of the normal are used
    case 0: n0 = na; n1 = nb; break;
    case 1: n0 = nc_; n1 = nb; break;
    case 2: n0 = -nc_; n1 = nb; break;
    case 4: n0 = na; n1 = -nc_; break;
    case 3: n0 = na; n1 = nc_; break;
    default: n0 = 0.0f; n1 = 0.0f;
  }
  const float epi[3] = {n1, -n0, 0.0f}, ver[3] = {n0, n1, 0.0f};
  const float u = kx - (float)(cms_init_cell(kx, F) * F), v = ky - (float)(cms_init_cell(ky, F) * F);
  const float OP[3] = {(float)((double)u - fx), (float)((double)v - fx), 0.0f};
  // Vec3f::dot: float, from 0
  float d_epi = 0.0f + OP[0] * epi[0]; d_epi = d_epi + OP[1] * epi[1]; d_epi = d_epi + OP[2] * epi[2];
  float d_ver = 0.0f + OP[0] * ver[0]; d_ver = d_ver + OP[1] * ver[1]; d_ver = d_ver + OP[2] * ver[2];
  float OO1 = (float)((double)d_epi / cms_init_dnorm3(epi)); if (OO1 < 0) OO1 = -OO1;
  const float CO1 = (float)sqrt((double)(OO1 * OO1) + fx * fx);
  float PO1 = (float)((double)d_ver / cms_init_dnorm3(ver)); if (PO1 < 0) PO1 = -PO1;
  const float tan1 = PO1 / CO1;
  const float tan2 = (PO1 + 1.0f) / CO1;
  const float tan3 = (tan2 - tan1) / (1.0f + tan1 * tan2);
  return 1.0f / sqrtf(1.0f / (tan3 * tan3) + 1.0f);
}

// CheckEssiential (:197-277) for one match: the two terms `thScore - chiSquare` and whether each is added (chiSquare <= th, NaN included as in the
// reference); returns bIn.  The caller adds term1 then term2, match after match: the score is that float sum in that order.
CMS_HD bool cms_init_check_terms(int F, const float* E, float sigma, const float* ray1, const float* ray2, const float* kp1, const float* kp2,
                                 float* term1, bool* add1, float* term2, bool* add2) {
  const float e11 = E[0], e12 = E[1], e13 = E[2], e21 = E[3], e22 = E[4], e23 = E[5], e31 = E[6], e32 = E[7], e33 = E[8];
  const float th = 3.841f, thScore = 5.991f;
  bool bIn = true;
  const float x1 = ray1[0], y1 = ray1[1], z1 = ray1[2];
  const float x2 = ray2[0], y2 = ray2[1], z2 = ray2[2];
  const float a2 = e11 * x1 + e12 * y1 + e13 * z1;
  const float b2 = e21 * x1 + e22 * y1 + e23 * z1;
  const float c2 = e31 * x1 + e32 * y1 + e33 * z1;
  const float num2 = a2 * x2 + b2 * y2 + c2 * z2;
  const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2 + c2 * c2);
  float unitVectorSigma = sigma * cms_init_vector_sigma(F, kp2[0], kp2[1], a2, b2, c2);
  float invSigmaSquare = 1.0f / (unitVectorSigma * unitVectorSigma);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) { bIn = false; *add1 = false; *term1 = 0.0f; }
  else { *add1 = true; *term1 = thScore - chiSquare1; }
  const float a1 = e11 * x2 + e21 * y2 + e31 * z2;
  const float b1 = e12 * x2 + e22 * y2 + e32 * z2;
  const float c1 = e13 * x2 + e23 * y2 + e33 * z2;
  const float num1 = a1 * x1 + b1 * y1 + c1 * z1;
  const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1 + c1 * c1);
  unitVectorSigma = sigma * cms_init_vector_sigma(F, kp1[0], kp1[1], a1, b1, c1);
  invSigmaSquare = 1.0f / (unitVectorSigma * unitVectorSigma);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) { bIn = false; *add2 = false; *term2 = 0.0f; }
  else { *add2 = true; *term2 = thScore - chiSquare2; }
  return bIn;
}

// DecomposeE (:501-521): t = u.col(2) / norm, R1 = u W vt, R2 = u Wt vt, each negated when its determinant (cv::determinant: double) is negative
CMS_HD double cms_init_det3(const float* m) {
  return (double)m[0] * ((double)m[4] * (double)m[8] - (double)m[5] * (double)m[7]) - (double)m[1] * ((double)m[3] * (double)m[8] - (double)m[5] * (double)m[6]) +
         (double)m[2] * ((double)m[3] * (double)m[7] - (double)m[4] * (double)m[6]);
}
CMS_HD void cms_init_decompose_e(const float* E, float* R1, float* R2, float* t) {
  float w[3], u[9], vt[9], tmp[9];
  cms_init_svd3(E, w, u, vt);
  t[0] = u[2]; t[1] = u[5]; t[2] = u[8];
  const float inv = (float)(1.0 / cms_init_dnorm3(t));
  t[0] = t[0] * inv; t[1] = t[1] * inv; t[2] = t[2] * inv;
  const float Wm[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};      // products with 0 and +-1: exact on either gemm path
  cms_init_gemm3(u, Wm, tmp);
  cms_init_gemm3(tmp, vt, R1);
  if (cms_init_det3(R1) < 0) {
    CMS_INIT_UNROLL
    for (int k = 0; k < 9; ++k) R1[k] = -R1[k];
  }
  cms_init_gemm3(u, Wt, tmp);
  cms_init_gemm3(tmp, vt, R2);
  if (cms_init_det3(R2) < 0) {
    CMS_INIT_UNROLL
    for (int k = 0; k < 9; ++k) R2[k] = -R2[k];
  }
}
// O2 = -R.t()*t (:420): a product with a transposed operand accumulates in double, alpha = -1 on the sum
CMS_HD void cms_init_o2(const float* R, const float* t, float* O2) {
  CMS_INIT_UNROLL
  for (int i = 0; i < 3; ++i) {
    double s = (double)R[i] * (double)t[0];
    s = s + (double)R[3 + i] * (double)t[1];
    s = s + (double)R[6 + i] * (double)t[2];
    O2[i] = (float)(s * -1.0);
  }
}

// one row of the triangulation system: r_a*(P.row(ia)+P.row(ib)) - (r_b+r_c)*P.row(ic) as two addWeighted passes, P = [R | t]
CMS_HD void cms_init_tri_row(const float* R, const float* t, int ia, int ib, int ic, float ra, float rb, float rc, float* out) {
  const float g = -(rb + rc);
  CMS_INIT_UNROLL
  for (int k = 0; k < 4; ++k) {
    const float va = k < 3 ? R[3 * ia + k] : t[ia], vb = k < 3 ? R[3 * ib + k] : t[ib], vc = k < 3 ? R[3 * ic + k] : t[ic];
    const float tmp = va * ra + vb * ra;
    out[k] = tmp * 1.0f + vc * g;
  }
}
// Triangulate (:378-393) with P1 = [Ra | ta], P2 = [Rb | tb]: x3D = vt.row(3)(0..2) / vt.row(3)(3)
CMS_HD void cms_init_triangulate(const float* ray1, const float* ray2, const float* Ra, const float* ta, const float* Rb, const float* tb, float* x3D) {
  float A[16], At[16], Vt[16];
  double W[4];
  cms_init_tri_row(Ra, ta, 1, 2, 0, ray1[0], ray1[1], ray1[2], A);
  cms_init_tri_row(Ra, ta, 0, 2, 1, ray1[1], ray1[0], ray1[2], A + 4);
  cms_init_tri_row(Rb, tb, 1, 2, 0, ray2[0], ray2[1], ray2[2], A + 8);
  cms_init_tri_row(Rb, tb, 0, 2, 1, ray2[1], ray2[0], ray2[2], A + 12);
  CMS_INIT_UNROLL
  for (int i = 0; i < 4; ++i)
    CMS_INIT_UNROLL
    for (int k = 0; k < 4; ++k) At[4 * i + k] = A[4 * k + i];
  cms_init_jacobi_reg<4>(At, Vt, W);
  const float inv_w = (float)(1.0 / (double)Vt[15]);
  x3D[0] = Vt[12] * inv_w; x3D[1] = Vt[13] * inv_w; x3D[2] = Vt[14] * inv_w;
}

// The body of CheckRT's loop (:429-485) for one inlier match.  Returns 1 when the point counts in nGood (p3d is then vP3D[first], *cosp is pushed to
// vCosParallax, *good is vbGood[first]), 0 when the loop `continue`s.
CMS_HD int cms_init_check_rt_match(int F, float cos_fov, float th2, const float* R, const float* t, const float* O2, const float* ray1, const float* ray2,
                                   const float* kp1, const float* kp2, float* p3d, float* cosp, int* good) {
  const float I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z3[3] = {0, 0, 0};
  float x[3];
  cms_init_triangulate(ray1, ray2, I3, z3, R, t, x);
  if (!cms_init_finite(x[0]) || !cms_init_finite(x[1]) || !cms_init_finite(x[2])) return 0;
  const float dist1 = (float)cms_init_dnorm3(x);                  // normal1 = p3dC1 - O1, O1 = 0
  const float n2[3] = {x[0] - O2[0], x[1] - O2[1], x[2] - O2[2]};
  const float dist2 = (float)cms_init_dnorm3(n2);
  const float cosParallax = (float)(cms_init_ddot3(x, n2) / (double)(dist1 * dist2));
  if (x[2] / dist1 <= cos_fov && (double)cosParallax < 0.99998) return 0;
  float p2[3];
  CMS_INIT_UNROLL
  for (int r = 0; r < 3; ++r) {                                   // R*p3dC1 + t: the small gemm, + C through double
    float s = R[3 * r] * x[0];
    s = s + R[3 * r + 1] * x[1];
    s = s + R[3 * r + 2] * x[2];
    p2[r] = (float)((double)s * 1.0 + (double)t[r] * 1.0);
  }
  if (p2[2] / dist2 <= cos_fov && (double)cosParallax < 0.99998) return 0;
  float imx, imy;
  track_rays_to_cubemap(F, x[0], x[1], x[2], imx, imy);
  const float squareError1 = (imx - kp1[0]) * (imx - kp1[0]) + (imy - kp1[1]) * (imy - kp1[1]);
  if (squareError1 > th2) return 0;
  track_rays_to_cubemap(F, p2[0], p2[1], p2[2], imx, imy);
  const float squareError2 = (imx - kp2[0]) * (imx - kp2[0]) + (imy - kp2[1]) * (imy - kp2[1]);
  if (squareError2 > th2) return 0;
  p3d[0] = x[0]; p3d[1] = x[1]; p3d[2] = x[2];
  *cosp = cosParallax;
  *good = (double)cosParallax < 0.99998 ? 1 : 0;
  return 1;
}

// vCosParallax is sorted and read at min(50, nGood - 1) (:490-493).  The order is made total so that the element is the same however it is
// selected: floats by value (-0 before +0), every NaN last and taken as one value.
CMS_HD unsigned cms_init_cos_key(float c) {
  if (c != c) return 0xffffffffu;
  unsigned u;
  __builtin_memcpy(&u, &c, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
CMS_HD float cms_init_cos_from_key(unsigned k) {
  unsigned u = k == 0xffffffffu ? 0x7fc00000u : ((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
  float c;
  __builtin_memcpy(&c, &u, 4);
  return c;
}

// th2 of CheckRT as ReconstructE passes it (:300): 4.0*mSigma2 in double, narrowed by the float parameter
CMS_HD float cms_init_th2(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }

// The eight draws of one iteration by the reference's swap-and-pop (cms_ransac_core.h)
CMS_HD void cms_init_resolve_draws(int N, const int* draws, int* idx) { cms_ransac_resolve_draws<8>(N, draws, idx); }

// ---- host only (plain `inline`: no device code is made of them): what the device leaves to the host.  Both the library's host side and the host
// build of the core call these.
// parallax = acos(vCosParallax[idx])*180/CV_PI (:493): acos on a float is the float overload, *180 in float, /CV_PI in double, stored in a float
inline float cms_init_parallax_deg(float cosine) { return (float)((double)(acosf(cosine) * 180.0f) / 3.1415926535897932384626433832795); }

// ReconstructE's decision (:305-375) from the four nGood, the four selected cosines and N = the number of inliers of the best hypothesis.
// Returns the winning hypothesis 0..3 (R1 t, R2 t, R1 -t, R2 -t) or -1; parallax[h] = 0 for nGood[h] == 0 (:495-496).
inline int cms_init_decide(const int* nGood, const float* cosines, int N, float* parallax) {
  for (int h = 0; h < 4; ++h) parallax[h] = nGood[h] > 0 ? cms_init_parallax_deg(cosines[h]) : 0.0f;
  int maxGood = nGood[3];
  for (int h = 2; h >= 0; --h) maxGood = nGood[h] > maxGood ? nGood[h] : maxGood;
  const int nNinety = static_cast<int>(0.9 * N);
  const int nMinGood = nNinety > 50 ? nNinety : 50;
  int nsimilar = 0;
  for (int h = 0; h < 4; ++h)
    if (nGood[h] > 0.7 * maxGood) nsimilar++;
  if (maxGood < nMinGood || nsimilar > 1) return -1;
  const float minParallax = 1.0f;
  if (maxGood == nGood[0]) { if (parallax[0] > minParallax) return 0; }
  else if (maxGood == nGood[1]) { if (parallax[1] > minParallax) return 1; }
  else if (maxGood == nGood[2]) { if (parallax[2] > minParallax) return 2; }
  else if (maxGood == nGood[3]) { if (parallax[3] > minParallax) return 3; }
  return -1;
}

#endif
