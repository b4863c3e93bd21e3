// cms_pnp_core.h -- the numeric core of PnPsolver (src/PnPsolver.cpp:312-343 and :385-961): EPnP on bearing vectors and the inlier test, ONE
// source for the host build (libcubemapslam_host.so: hm_pnp_iterate_host, the definition of record) and for the gfx950 kernels
// (cms_pnp_kernels.hip).  This header compiles under g++ as it stands (tests/emu/pnp_core_emu.cpp includes it): there is no text to paste and
// therefore no host-emulation marker in it.
//
// Determinism contract: plain IEEE + - * / sqrt in double (float where the reference computes in float), in the order this source fixes; both
// builds use -ffp-contract=off.  No fma(), no reciprocal / rsqrt builtins, no libm beyond sqrt / fabs, no allocation: every array arrives as a
// pointer (the kernels hand over LDS for mtm / ut).  The same inputs give the same bits from g++ and from hipcc.
//
// The SVD.  The reference calls OpenCV: cvSVD three times (3x3 PCA, 12x12 MtM with U_T, 3x3 ABt with U and V), cvInvert(CV_SVD) once and
// cvSolve(CV_SVD) three times.  All seven go through cms_pnp_jacobi here: a one-sided Hestenes Jacobi on the columns of A (the algorithm of OpenCV
// 2.4 / 3.2's JacobiSVDImpl_ for CV_64F without LAPACK, recalled and unpinned -- SURVEY.md Appendix C convention), singular values descending,
// at most 30 sweeps (a NaN input terminates), pair order (0,1) (0,2) ... (n-2,n-1), every dot product summed upwards.  For the two symmetric
// matrices (PCA, MtM) the rows handed on as `uct` / `ut` are the rows of Vt: V is a product of rotations, so its rows stay orthonormal also inside
// a null space (a four-point MtM has one of dimension >= 4), where A v / sigma is undefined.  Back-substitution and pseudo-inverse drop singular
// values <= 2 * DBL_EPSILON * sum(w).
//
// Degenerate inputs: qr_solve with eta == 0 gives a zero update (the reference returns with X stale); NaN / inf from a zero betas[0] flow through,
// every comparison with them is false as in the reference; nothing traps, nothing loops.
#ifndef CMS_PNP_CORE_H
#define CMS_PNP_CORE_H
#include <float.h>
#include <math.h>
#include "cms_cubemap_project.h"      // CMS_HD, track_rays_to_cubemap = CamModelGeneral::TransformRaysToCubemap
#include "cms_ransac_core.h"          // cms_ransac_resolve_draws: the draws of one iteration

// What compute_pose leaves behind for a caller that wants to see the stages (the CPU tests); the kernels pass NULL.
struct CmsPnpStages {
  double cws[12], dc[3], uct[9];      // control points, PCA singular values, PCA vectors (rows)
  double d[12];                       // singular values of MtM (ut itself is the caller's array)
  double l_6x10[60], rho[6];
  double betas0[3][4], betas[3][4];   // find_betas_approx_1/2/3, before and after gauss_newton
  double Rs[3][9], ts[3][3], rep[3];
  int chosen;                         // 1, 2 or 3
};

// One-sided Jacobi SVD of A (m x n, m >= n).  In: At, n rows of length m = the columns of A.  Out: row k of At = A v_k = w[k] u_k, row k of Vt
// (n x n) = v_k, w descending.
CMS_HD void cms_pnp_jacobi(int m, int n, double* At, double* Vt, double* w) {
  const double eps = DBL_EPSILON * 10;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) Vt[i * n + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    int changed = 0;
    for (int i = 0; i < n - 1; ++i)
      for (int j = i + 1; j < n; ++j) {
        double* Ai = At + i * m;
        double* Aj = At + j * m;
        double a = 0.0, b = 0.0, p = 0.0;
        for (int k = 0; k < m; ++k) { a += Ai[k] * Ai[k]; b += Aj[k] * Aj[k]; p += Ai[k] * Aj[k]; }
        if (fabs(p) <= eps * sqrt(a * b)) continue;
        p *= 2.0;
        const double beta = a - b, gamma = sqrt(p * p + beta * beta);
        double c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = sqrt(delta / gamma);
          c = p / (gamma * s * 2.0);
        } else {
          c = sqrt((gamma + beta) / (gamma * 2.0));
          s = p / (gamma * c * 2.0);
        }
        for (int k = 0; k < m; ++k) { const double t0 = c * Ai[k] + s * Aj[k], t1 = c * Aj[k] - s * Ai[k]; Ai[k] = t0; Aj[k] = t1; }
        double* Vi = Vt + i * n;
        double* Vj = Vt + j * n;
        for (int k = 0; k < n; ++k) { const double t0 = c * Vi[k] + s * Vj[k], t1 = c * Vj[k] - s * Vi[k]; Vi[k] = t0; Vj[k] = t1; }
        changed = 1;
      }
    if (!changed) break;
  }
  for (int i = 0; i < n; ++i) {
    double sd = 0.0;
    for (int k = 0; k < m; ++k) sd += At[i * m + k] * At[i * m + k];
    w[i] = sqrt(sd);
  }
  for (int i = 0; i < n - 1; ++i) {      // selection sort, first maximum
    int j = i;
    for (int k = i + 1; k < n; ++k)
      if (w[j] < w[k]) j = k;
    if (i != j) {
      const double tw = w[i]; w[i] = w[j]; w[j] = tw;
      for (int k = 0; k < m; ++k) { const double tv = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = tv; }
      for (int k = 0; k < n; ++k) { const double tv = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = tv; }
    }
  }
}

CMS_HD double cms_pnp_svd_threshold(int n, const double* w) {
  double sum = 0.0;
  for (int k = 0; k < n; ++k) sum += w[k];
  return 2.0 * DBL_EPSILON * sum;
}

// cvSolve(A, b, x, CV_SVD), A m x n row major, m <= 6, n <= 5
CMS_HD void cms_pnp_svd_solve(int m, int n, const double* A, const double* b, double* x) {
  double At[30], Vt[25], w[5];
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < n; ++j) At[j * m + i] = A[i * n + j];
  cms_pnp_jacobi(m, n, At, Vt, w);
  const double thr = cms_pnp_svd_threshold(n, w);
  for (int j = 0; j < n; ++j) x[j] = 0.0;
  for (int k = 0; k < n; ++k) {
    if (!(w[k] > thr)) continue;
    double s = 0.0;
    for (int i = 0; i < m; ++i) s += At[k * m + i] * b[i];
    s = s / (w[k] * w[k]);
    for (int j = 0; j < n; ++j) x[j] += s * Vt[k * n + j];
  }
}

// cvInvert(A, inv, CV_SVD), 3 x 3 row major
CMS_HD void cms_pnp_svd_invert3(const double* A, double* inv) {
  double At[9], Vt[9], w[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) At[j * 3 + i] = A[i * 3 + j];
  cms_pnp_jacobi(3, 3, At, Vt, w);
  const double thr = cms_pnp_svd_threshold(3, w);
  for (int i = 0; i < 9; ++i) inv[i] = 0.0;
  for (int k = 0; k < 3; ++k) {
    if (!(w[k] > thr)) continue;
    const double w2 = w[k] * w[k];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) inv[3 * i + j] += Vt[3 * k + i] * At[3 * k + j] / w2;
  }
}

CMS_HD double cms_pnp_dist2(const double* p1, const double* p2) {
  return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}
CMS_HD double cms_pnp_dot(const double* v1, const double* v2) { return v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]; }

// choose_control_points (:385-419); cws is 4 x 3
CMS_HD void cms_pnp_choose_control_points(int n, const double* pws, double* cws, double* dc, double* uct) {
  cws[0] = cws[1] = cws[2] = 0;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < 3; j++) cws[j] += pws[3 * i + j];
  for (int j = 0; j < 3; j++) cws[j] /= n;
  double pw0tpw0[9];
  for (int a = 0; a < 9; ++a) pw0tpw0[a] = 0.0;
  for (int i = 0; i < n; i++) {      // cvMulTransposed(PW0, &PW0tPW0, 1): rows summed upwards
    double r[3];
    for (int j = 0; j < 3; j++) r[j] = pws[3 * i + j] - cws[j];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) pw0tpw0[3 * a + b] += r[a] * r[b];
  }
  cms_pnp_jacobi(3, 3, pw0tpw0, uct, dc);      // symmetric: its columns are its rows
  for (int i = 1; i < 4; i++) {
    const double k = sqrt(dc[i - 1] / n);
    for (int j = 0; j < 3; j++) cws[3 * i + j] = cws[j] + k * uct[3 * (i - 1) + j];
  }
}

// compute_barycentric_coordinates (:421-444)
CMS_HD void cms_pnp_barycentric(int n, const double* pws, const double* cws, double* alphas) {
  double cc[9], ci[9];
  for (int i = 0; i < 3; i++)
    for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[3 * j + i] - cws[i];
  cms_pnp_svd_invert3(cc, ci);
  for (int i = 0; i < n; i++) {
    const double* pi = pws + 3 * i;
    double* a = alphas + 4 * i;
    for (int j = 0; j < 3; j++)
      a[1 + j] = ci[3 * j] * (pi[0] - cws[0]) + ci[3 * j + 1] * (pi[1] - cws[1]) + ci[3 * j + 2] * (pi[2] - cws[2]);
    a[0] = 1.0f - a[1] - a[2] - a[3];
  }
}

// fill_M_with_bearing (:447-462): the two rows of one correspondence, bearing (r, s, t)
CMS_HD void cms_pnp_fill_M_rows(const double* as, double r, double s, double t, double* M1, double* M2) {
  for (int i = 0; i < 4; i++) {
    M1[3 * i] = as[i] * (s + t);
    M1[3 * i + 1] = -as[i] * r;
    M1[3 * i + 2] = -as[i] * r;
    M2[3 * i] = -as[i] * s;
    M2[3 * i + 1] = as[i] * (r + t);
    M2[3 * i + 2] = -as[i] * s;
  }
}

// cvMulTransposed(M, &MtM, 1) without M: the rows of M are formed and summed in their order (row 2i, then 2i + 1)
CMS_HD void cms_pnp_mtm(int n, const double* alphas, const double* bearings, double* mtm) {
  for (int a = 0; a < 144; ++a) mtm[a] = 0.0;
  for (int i = 0; i < n; i++) {
    double M1[12], M2[12];
    cms_pnp_fill_M_rows(alphas + 4 * i, bearings[3 * i], bearings[3 * i + 1], bearings[3 * i + 2], M1, M2);
    for (int a = 0; a < 12; ++a)
      for (int b = 0; b < 12; ++b) mtm[12 * a + b] += M1[a] * M1[b];
    for (int a = 0; a < 12; ++a)
      for (int b = 0; b < 12; ++b) mtm[12 * a + b] += M2[a] * M2[b];
  }
}

// compute_L_6x10 (:771-811)
CMS_HD void cms_pnp_compute_L_6x10(const double* ut, double* l_6x10) {
  const double* v[4];
  v[0] = ut + 12 * 11;
  v[1] = ut + 12 * 10;
  v[2] = ut + 12 * 9;
  v[3] = ut + 12 * 8;
  double dv[4][6][3];
  for (int i = 0; i < 4; i++) {
    int a = 0, b = 1;
    for (int j = 0; j < 6; j++) {
      dv[i][j][0] = v[i][3 * a] - v[i][3 * b];
      dv[i][j][1] = v[i][3 * a + 1] - v[i][3 * b + 1];
      dv[i][j][2] = v[i][3 * a + 2] - v[i][3 * b + 2];
      b++;
      if (b > 3) { a++; b = a + 1; }
    }
  }
  for (int i = 0; i < 6; i++) {
    double* row = l_6x10 + 10 * i;
    row[0] = cms_pnp_dot(dv[0][i], dv[0][i]);
    row[1] = 2.0f * cms_pnp_dot(dv[0][i], dv[1][i]);
    row[2] = cms_pnp_dot(dv[1][i], dv[1][i]);
    row[3] = 2.0f * cms_pnp_dot(dv[0][i], dv[2][i]);
    row[4] = 2.0f * cms_pnp_dot(dv[1][i], dv[2][i]);
    row[5] = cms_pnp_dot(dv[2][i], dv[2][i]);
    row[6] = 2.0f * cms_pnp_dot(dv[0][i], dv[3][i]);
    row[7] = 2.0f * cms_pnp_dot(dv[1][i], dv[3][i]);
    row[8] = 2.0f * cms_pnp_dot(dv[2][i], dv[3][i]);
    row[9] = cms_pnp_dot(dv[3][i], dv[3][i]);
  }
}

// compute_rho (:813-821)
CMS_HD void cms_pnp_compute_rho(const double* cws, double* rho) {
  rho[0] = cms_pnp_dist2(cws, cws + 3);
  rho[1] = cms_pnp_dist2(cws, cws + 6);
  rho[2] = cms_pnp_dist2(cws, cws + 9);
  rho[3] = cms_pnp_dist2(cws + 3, cws + 6);
  rho[4] = cms_pnp_dist2(cws + 3, cws + 9);
  rho[5] = cms_pnp_dist2(cws + 6, cws + 9);
}

// find_betas_approx_1 (:678-705): betas10 = [B11 B12 B22 B13 B23 B33 B14 B24 B34 B44], approx_1 = [B11 B12 B13 B14]
CMS_HD void cms_pnp_find_betas_approx_1(const double* l_6x10, const double* rho, double* betas) {
  double l_6x4[24], b4[4];
  for (int i = 0; i < 6; i++) {
    l_6x4[4 * i] = l_6x10[10 * i];
    l_6x4[4 * i + 1] = l_6x10[10 * i + 1];
    l_6x4[4 * i + 2] = l_6x10[10 * i + 3];
    l_6x4[4 * i + 3] = l_6x10[10 * i + 6];
  }
  cms_pnp_svd_solve(6, 4, l_6x4, rho, b4);
  if (b4[0] < 0) {
    betas[0] = sqrt(-b4[0]);
    betas[1] = -b4[1] / betas[0];
    betas[2] = -b4[2] / betas[0];
    betas[3] = -b4[3] / betas[0];
  } else {
    betas[0] = sqrt(b4[0]);
    betas[1] = b4[1] / betas[0];
    betas[2] = b4[2] / betas[0];
    betas[3] = b4[3] / betas[0];
  }
}

// find_betas_approx_2 (:710-737): approx_2 = [B11 B12 B22]
CMS_HD void cms_pnp_find_betas_approx_2(const double* l_6x10, const double* rho, double* betas) {
  double l_6x3[18], b3[3];
  for (int i = 0; i < 6; i++) {
    l_6x3[3 * i] = l_6x10[10 * i];
    l_6x3[3 * i + 1] = l_6x10[10 * i + 1];
    l_6x3[3 * i + 2] = l_6x10[10 * i + 2];
  }
  cms_pnp_svd_solve(6, 3, l_6x3, rho, b3);
  if (b3[0] < 0) {
    betas[0] = sqrt(-b3[0]);
    betas[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0;
  } else {
    betas[0] = sqrt(b3[0]);
    betas[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;
  }
  if (b3[1] < 0) betas[0] = -betas[0];
  betas[2] = 0.0;
  betas[3] = 0.0;
}

// find_betas_approx_3 (:742-769): approx_3 = [B11 B12 B22 B13 B23]
CMS_HD void cms_pnp_find_betas_approx_3(const double* l_6x10, const double* rho, double* betas) {
  double l_6x5[30], b5[5];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 5; j++) l_6x5[5 * i + j] = l_6x10[10 * i + j];
  cms_pnp_svd_solve(6, 5, l_6x5, rho, b5);
  if (b5[0] < 0) {
    betas[0] = sqrt(-b5[0]);
    betas[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
  } else {
    betas[0] = sqrt(b5[0]);
    betas[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
  }
  if (b5[1] < 0) betas[0] = -betas[0];
  betas[2] = b5[3] / betas[0];
  betas[3] = 0.0;
}

// compute_A_and_b_gauss_newton (:823-849)
CMS_HD void cms_pnp_A_and_b_gauss_newton(const double* l_6x10, const double* rho, const double* betas, double* A, double* b) {
  for (int i = 0; i < 6; i++) {
    const double* rowL = l_6x10 + i * 10;
    double* rowA = A + i * 4;
    rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
    rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
    rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
    rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
    b[i] = rho[i] -
           (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
            rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] + rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
            rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
  }
}

// qr_solve (:871-961), the Householder code as written; nr x nc with nr <= 6.  eta == 0: X = 0.
CMS_HD void cms_pnp_qr_solve(int nr, int nc, double* pA, double* pb, double* pX) {
  double A1[6], A2[6];
  double* ppAkk = pA;
  for (int k = 0; k < nc; k++) {
    double* ppAik = ppAkk;
    double eta = fabs(*ppAik);
    for (int i = k + 1; i < nr; i++) {
      const double elt = fabs(*ppAik);
      if (eta < elt) eta = elt;
      ppAik += nc;
    }
    if (eta == 0) {
      for (int j = 0; j < nc; j++) pX[j] = 0.0;
      return;
    } else {
      double* ppAik = ppAkk;
      double sum = 0.0;
      const double inv_eta = 1. / eta;
      for (int i = k; i < nr; i++) {
        *ppAik *= inv_eta;
        sum += *ppAik * *ppAik;
        ppAik += nc;
      }
      double sigma = sqrt(sum);
      if (*ppAkk < 0) sigma = -sigma;
      *ppAkk += sigma;
      A1[k] = sigma * *ppAkk;
      A2[k] = -eta * sigma;
      for (int j = k + 1; j < nc; j++) {
        double* ppAik = ppAkk;
        double sum = 0;
        for (int i = k; i < nr; i++) {
          sum += *ppAik * ppAik[j - k];
          ppAik += nc;
        }
        const double tau = sum / A1[k];
        ppAik = ppAkk;
        for (int i = k; i < nr; i++) {
          ppAik[j - k] -= tau * *ppAik;
          ppAik += nc;
        }
      }
    }
    ppAkk += nc + 1;
  }
  // b <- Qt b
  double* ppAjj = pA;
  for (int j = 0; j < nc; j++) {
    double* ppAij = ppAjj;
    double tau = 0;
    for (int i = j; i < nr; i++) {
      tau += *ppAij * pb[i];
      ppAij += nc;
    }
    tau /= A1[j];
    ppAij = ppAjj;
    for (int i = j; i < nr; i++) {
      pb[i] -= tau * *ppAij;
      ppAij += nc;
    }
    ppAjj += nc + 1;
  }
  // X = R-1 b
  pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
  for (int i = nc - 2; i >= 0; i--) {
    double* ppAij = pA + i * nc + (i + 1);
    double sum = 0;
    for (int j = i + 1; j < nc; j++) {
      sum += *ppAij * pX[j];
      ppAij++;
    }
    pX[i] = (pb[i] - sum) / A2[i];
  }
}

// gauss_newton (:851-869)
CMS_HD void cms_pnp_gauss_newton(const double* l_6x10, const double* rho, double* betas) {
  double a[24], b[6], x[4];
  for (int k = 0; k < 5; k++) {
    cms_pnp_A_and_b_gauss_newton(l_6x10, rho, betas, a, b);
    cms_pnp_qr_solve(6, 4, a, b, x);
    for (int i = 0; i < 4; i++) betas[i] += x[i];
  }
}

// compute_ccs (:464-475), compute_pcs (:477-486), solve_for_sign (:647-660: the first point's z)
CMS_HD void cms_pnp_ccs_pcs(int n, const double* betas, const double* ut, const double* alphas, double* ccs, double* pcs) {
  for (int i = 0; i < 12; i++) ccs[i] = 0.0f;
  for (int i = 0; i < 4; i++) {
    const double* v = ut + 12 * (11 - i);
    for (int j = 0; j < 4; j++)
      for (int k = 0; k < 3; k++) ccs[3 * j + k] += betas[i] * v[3 * j + k];
  }
  for (int i = 0; i < n; i++) {
    const double* a = alphas + 4 * i;
    double* pc = pcs + 3 * i;
    for (int j = 0; j < 3; j++) pc[j] = a[0] * ccs[j] + a[1] * ccs[3 + j] + a[2] * ccs[6 + j] + a[3] * ccs[9 + j];
  }
  if (pcs[2] < 0.0) {
    for (int i = 0; i < 12; i++) ccs[i] = -ccs[i];
    for (int i = 0; i < 3 * n; i++) pcs[i] = -pcs[i];
  }
}

// estimate_R_and_t (:580-638); R is 3 x 3 row major
CMS_HD void cms_pnp_estimate_R_and_t(int n, const double* pws, const double* pcs, double* R, double* t) {
  double pc0[3], pw0[3];
  pc0[0] = pc0[1] = pc0[2] = 0.0;
  pw0[0] = pw0[1] = pw0[2] = 0.0;
  for (int i = 0; i < n; i++) {
    const double* pc = pcs + 3 * i;
    const double* pw = pws + 3 * i;
    for (int j = 0; j < 3; j++) {
      pc0[j] += pc[j];
      pw0[j] += pw[j];
    }
  }
  for (int j = 0; j < 3; j++) {
    pc0[j] /= n;
    pw0[j] /= n;
  }
  double abt[9], abt_d[3], abt_u[9], abt_v[9], at[9], vt[9];
  for (int i = 0; i < 9; i++) abt[i] = 0.0;
  for (int i = 0; i < n; i++) {
    const double* pc = pcs + 3 * i;
    const double* pw = pws + 3 * i;
    for (int j = 0; j < 3; j++) {
      abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
      abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
      abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
    }
  }
  // cvSVD(&ABt, &ABt_D, &ABt_U, &ABt_V): U[i][k] = (A v_k)[i] / w[k], V[j][k] = v_k[j]; a direction without a singular value (coplanar points)
  // is the cross product of the other two
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) at[3 * j + i] = abt[3 * i + j];
  cms_pnp_jacobi(3, 3, at, vt, abt_d);
  const double thr = cms_pnp_svd_threshold(3, abt_d);
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i) {
      abt_u[3 * i + k] = abt_d[k] > thr ? at[3 * k + i] / abt_d[k] : 0.0;
      abt_v[3 * i + k] = vt[3 * k + i];
    }
  if (abt_d[1] > thr && !(abt_d[2] > thr)) {
    abt_u[2] = abt_u[3] * abt_u[7] - abt_u[6] * abt_u[4];
    abt_u[5] = abt_u[6] * abt_u[1] - abt_u[0] * abt_u[7];
    abt_u[8] = abt_u[0] * abt_u[4] - abt_u[3] * abt_u[1];
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = cms_pnp_dot(abt_u + 3 * i, abt_v + 3 * j);
  const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
  if (det < 0) {
    R[6] = -R[6];
    R[7] = -R[7];
    R[8] = -R[8];
  }
  t[0] = pc0[0] - cms_pnp_dot(R, pw0);
  t[1] = pc0[1] - cms_pnp_dot(R + 3, pw0);
  t[2] = pc0[2] - cms_pnp_dot(R + 6, pw0);
}

// reprojection_error (:561-578): the camera-frame point is narrowed to float by TransformRaysToCubemap's parameters
CMS_HD double cms_pnp_reprojection_error(int n, int F, const double* pws, const double* us, const double* R, const double* t) {
  double sum2 = 0.0;
  for (int i = 0; i < n; i++) {
    const double* pw = pws + 3 * i;
    const double Xc = cms_pnp_dot(R, pw) + t[0];
    const double Yc = cms_pnp_dot(R + 3, pw) + t[1];
    const double Zc = cms_pnp_dot(R + 6, pw) + t[2];
    float ue, ve;
    track_rays_to_cubemap(F, (float)Xc, (float)Yc, (float)Zc, ue, ve);
    const double u = us[2 * i], v = us[2 * i + 1];
    sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
  }
  return sum2 / n;
}

// compute_R_and_t (:662-673)
CMS_HD double cms_pnp_compute_R_and_t(int n, int F, const double* pws, const double* us, const double* alphas, double* pcs, const double* ut,
                                      const double* betas, double* R, double* t) {
  double ccs[12];
  cms_pnp_ccs_pcs(n, betas, ut, alphas, ccs, pcs);
  cms_pnp_estimate_R_and_t(n, pws, pcs, R, t);
  return cms_pnp_reprojection_error(n, F, pws, us, R, t);
}

// The part of compute_pose behind the eigenvectors of MtM (:507-535).  ut: 12 x 12, rows = singular vectors, descending
CMS_HD double cms_pnp_pose_from_ut(int n, int F, const double* pws, const double* us, const double* alphas, double* pcs, const double* cws,
                                   const double* ut, double* R, double* t, CmsPnpStages* st) {
  double l_6x10[60], rho[6];
  cms_pnp_compute_L_6x10(ut, l_6x10);
  cms_pnp_compute_rho(cws, rho);
  double Betas[4][4], rep_errors[4];
  double Rs[4][9], ts[4][3];
  for (int s = 1; s <= 3; ++s) {
    if (s == 1) cms_pnp_find_betas_approx_1(l_6x10, rho, Betas[1]);
    else if (s == 2) cms_pnp_find_betas_approx_2(l_6x10, rho, Betas[2]);
    else cms_pnp_find_betas_approx_3(l_6x10, rho, Betas[3]);
    if (st)
      for (int i = 0; i < 4; ++i) st->betas0[s - 1][i] = Betas[s][i];
    cms_pnp_gauss_newton(l_6x10, rho, Betas[s]);
    rep_errors[s] = cms_pnp_compute_R_and_t(n, F, pws, us, alphas, pcs, ut, Betas[s], Rs[s], ts[s]);
  }
  int N = 1;
  if (rep_errors[2] < rep_errors[1]) N = 2;
  if (rep_errors[3] < rep_errors[N]) N = 3;
  for (int i = 0; i < 9; ++i) R[i] = Rs[N][i];
  for (int i = 0; i < 3; ++i) t[i] = ts[N][i];
  if (st) {
    for (int i = 0; i < 60; ++i) st->l_6x10[i] = l_6x10[i];
    for (int i = 0; i < 6; ++i) st->rho[i] = rho[i];
    for (int s = 0; s < 3; ++s) {
      for (int i = 0; i < 4; ++i) st->betas[s][i] = Betas[s + 1][i];
      for (int i = 0; i < 9; ++i) st->Rs[s][i] = Rs[s + 1][i];
      for (int i = 0; i < 3; ++i) st->ts[s][i] = ts[s + 1][i];
      st->rep[s] = rep_errors[s + 1];
    }
    st->chosen = N;
  }
  return rep_errors[N];
}

// compute_pose (:488-536).  pws 3n, us 2n, bearings 3n: the correspondences as add_bearing_correspondence stores them; alphas 4n, pcs 3n,
// mtm 144 and ut 144 are the caller's scratch (ut holds the eigenvectors on return).  R 3 x 3 row major, t 3.
CMS_HD double cms_pnp_compute_pose(int n, int F, const double* pws, const double* us, const double* bearings, double* alphas, double* pcs,
                                   double* mtm, double* ut, double* R, double* t, CmsPnpStages* st) {
  double cws[12], dc[3], uct[9], d[12];
  cms_pnp_choose_control_points(n, pws, cws, dc, uct);
  cms_pnp_barycentric(n, pws, cws, alphas);
  cms_pnp_mtm(n, alphas, bearings, mtm);
  cms_pnp_jacobi(12, 12, mtm, ut, d);      // symmetric: its columns are its rows
  if (st) {
    for (int i = 0; i < 12; ++i) { st->cws[i] = cws[i]; st->d[i] = d[i]; }
    for (int i = 0; i < 3; ++i) st->dc[i] = dc[i];
    for (int i = 0; i < 9; ++i) st->uct[i] = uct[i];
  }
  return cms_pnp_pose_from_ut(n, F, pws, us, alphas, pcs, cws, ut, R, t, st);
}

// CheckInliers (:312-343) for one correspondence: the camera-frame point in double (double x float), narrowed once; the face is not looked at
// -- ue, ve are whatever TransformRaysToCubemap left (the in-face values for a point in a branch but outside the face, -1 in no branch); float
// differences, float error2 < mvMaxError[i], strictly
CMS_HD bool cms_pnp_is_inlier(int F, const double* R, const double* t, const float* P3Dw, const float* P2D, float max_error) {
  const float Xc = (float)(R[0] * P3Dw[0] + R[1] * P3Dw[1] + R[2] * P3Dw[2] + t[0]);
  const float Yc = (float)(R[3] * P3Dw[0] + R[4] * P3Dw[1] + R[5] * P3Dw[2] + t[1]);
  const float Zc = (float)(R[6] * P3Dw[0] + R[7] * P3Dw[1] + R[8] * P3Dw[2] + t[2]);
  float ue, ve;
  track_rays_to_cubemap(F, Xc, Yc, Zc, ue, ve);
  const float distX = P2D[0] - ue;
  const float distY = P2D[1] - ve;
  const float error2 = distX * distX + distY * distY;
  return error2 < max_error;
}

// The four draws of one iteration by the reference's swap-and-pop (cms_ransac_core.h)
CMS_HD void cms_pnp_resolve_draws(int N, const int* draws, int* idx) { cms_ransac_resolve_draws<4>(N, draws, idx); }

#endif
