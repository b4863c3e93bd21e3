// cms_ess_graph_core.h -- the numeric core of Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:623-886): g2o::Sim3::log (sim3.h:148-225),
// EdgeSim3 (types_seven_dof_expmap.h:106-114), g2o's numeric linearizeOplus on both vertices (core/base_binary_edge.hpp:131-204), the quadratic form
// with identity information and no robust kernel, a block LDL^T inside the row envelope for the 7N x 7N system, and the Levenberg step with
// setUserLambdaInit.  ONE source for the host build (libcubemapslam_host.so: hm_essential_graph_optimize_host, the definition of record) and for the
// gfx950 kernel (cms_ess_graph_kernels.hip).  It sits on cms_sim3_opt_core.h (CmsS3, exp, oplus, mul, inverse, map, the Levenberg judge / stop, the
// slot tree) and keeps that header's determinism contract: plain IEEE + - * / sqrt in the order this source fixes, -ffp-contract=off, no libm.
//
//   log / acos  cms_det_log and cms_det_acos are this header's own: table-free reductions and Horner forms whose coefficients are quotients of
//               small integers (exact operands, one IEEE division each), so g++ and hipcc give the same bits
//   edges       edge e = (v0, v1, kind): measurement C = Sj * Si^-1 with i = v0, j = v1, taken from Scw (kind 0, the loop-connection edges of
//               :693-722) or from Snc (kind 1, :724-825), formed once per call; error = log(C * S[v0] * S[v1]^-1)
//   jacobian    fourteen perturbed estimates per free vertex (oplus(+-1e-9 e_d)), column d = (1 / 2e-9) * (e+ - e-); nothing for the fixed vertex
//   unknowns    the non-fixed vertices in ascending vertex index ("free index" f)
//   assembly    diagonal block and b of f: sums over the incident edges in ascending edge index; block (i, j), j < i: the sum over the edges of
//               that pair in ascending edge index (two edges on one pair are legal)
//   sums        chi2: edge e adds into slot e mod 256 in ascending e; the scale sum: free vertex f adds its x.(lambda x + b) into slot f mod 256;
//               the slots are folded by cms_s3o_tree
//   solve       first[i] = the lowest free neighbour of i (or i); stored blocks (i, j), first[i] <= j <= i.  Right-looking, unpivoted: at pivot j
//               the diagonal block is factored as cms_s3o_solve7 factors, the blocks of column j are scaled, the trailing blocks (i, k),
//               j < k <= i, of those rows take X(i,j) D_j X(k,j)^T.  Every block receives its updates in ascending j.  A zero or non-finite pivot
//               is a failed solve: the update is zero and the trial is rejected
#ifndef CMS_ESS_GRAPH_CORE_H
#define CMS_ESS_GRAPH_CORE_H
#include "cms_sim3_opt_core.h"

// ---- log(x), x > 0: x = m 2^k with m in [sqrt(1/2), sqrt(2)); f = m - 1 is exact, s = f / (2 + f), log m = 2 s (1 + s^2/3 + s^4/5 + ...)
// (|s| <= 0.1716: the term behind s^26 / 27 is below 1e-21); k ln 2 in two parts as cms_det_exp has it
CMS_HD double cms_det_log(double x) {
  if (!(x == x) || x < 0.0) return __builtin_nan("");
  if (x == 0.0) return -__builtin_inf();
  if (x == __builtin_inf()) return x;
  int k = 0;
  if (x < 2.2250738585072014e-308) { x = x * 18014398509481984.0; k = -54; }      // subnormal: times 2^54, exact
  unsigned long long bits;
  __builtin_memcpy(&bits, &x, 8);
  k += (int)((bits >> 52) & 0x7ff) - 1023;
  bits = (bits & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL;
  double m;
  __builtin_memcpy(&m, &bits, 8);                                                  // [1, 2)
  if (m > 1.4142135623730951) { m = m * 0.5; k += 1; }
  const double f = m - 1.0;
  const double s = f / (2.0 + f), s2 = s * s;
  double p = 1.0 / 27.0;
  for (int n = 12; n >= 1; --n) p = p * s2 + 1.0 / (double)(2 * n + 1);          // 1/25 ... 1/3
  const double lm = 2.0 * s + (2.0 * s) * (s2 * p);
  const double kd = (double)k;
  return kd * 6.93147180369123816490e-01 + (kd * 1.90821492927058770002e-10 + lm);
}
// asin(z), |z| <= 0.5: z (1 + r1 z^2 (1 + r2 z^2 (1 + ...))), r_n = (2n - 1)^2 / (2n (2n + 1)): the nested form of the Taylor series, 30 terms
// (the first one left out is below 0.25^31 / 60)
CMS_HD double cms_det_asin_half(double z) {
  const double z2 = z * z;
  double p = 1.0;
  for (int n = 30; n >= 1; --n) p = 1.0 + (((double)((2 * n - 1) * (2 * n - 1)) / (double)(2 * n * (2 * n + 1))) * z2) * p;
  return z * p;
}
// acos(d), |d| <= 1: 2 asin(sqrt((1 - d) / 2)) above 0.5, pi - 2 asin(sqrt((1 + d) / 2)) below -0.5, pi/2 - asin(d) between; pi in two parts
CMS_HD double cms_det_acos(double d) {
  if (!(fabs(d) <= 1.0)) return __builtin_nan("");
  if (d > 0.5) return 2.0 * cms_det_asin_half(sqrt((1.0 - d) * 0.5));
  if (d < -0.5) return (3.14159265358979311600e+00 - 2.0 * cms_det_asin_half(sqrt((1.0 + d) * 0.5))) + 1.22464679914735317723e-16;
  return (1.57079632679489655800e+00 - cms_det_asin_half(d)) + 6.12323399573676588613e-17;
}

// W.lu().solve(t), 3 x 3 row major.  Eigen's PartialPivLU: in column k the pivot is the entry of largest magnitude among rows k.., the FIRST such
// row on a tie; the rows are exchanged, the column below the pivot is divided by it, and the trailing block takes a(i,j) -= a(i,k) a(k,j).  The
// solve permutes t, runs the unit lower triangle forwards and the upper triangle backwards with one division per row
CMS_HD void cms_eg_lu3_solve(const double* W, const double* t, double* x) {
  double a[9], b[3] = {t[0], t[1], t[2]};
  for (int i = 0; i < 9; ++i) a[i] = W[i];
  for (int k = 0; k < 3; ++k) {
    int piv = k;
    double best = fabs(a[3 * k + k]);
    for (int i = k + 1; i < 3; ++i) { const double v = fabs(a[3 * i + k]); if (v > best) { best = v; piv = i; } }
    if (piv != k) {
      for (int j = 0; j < 3; ++j) { const double v = a[3 * k + j]; a[3 * k + j] = a[3 * piv + j]; a[3 * piv + j] = v; }
      const double v = b[k]; b[k] = b[piv]; b[piv] = v;
    }
    for (int i = k + 1; i < 3; ++i) {
      a[3 * i + k] = a[3 * i + k] / a[3 * k + k];
      for (int j = k + 1; j < 3; ++j) a[3 * i + j] = a[3 * i + j] - a[3 * i + k] * a[3 * k + j];
    }
  }
  b[1] = b[1] - a[3] * b[0];
  b[2] = (b[2] - a[6] * b[0]) - a[7] * b[1];
  x[2] = b[2] / a[8];
  x[1] = (b[1] - a[5] * x[2]) / a[4];
  x[0] = ((b[0] - a[1] * x[1]) - a[2] * x[2]) / a[0];
}

// Sim3::log() (sim3.h:148-225): u = omega | upsilon | sigma
CMS_HD void cms_eg_log(const CmsS3& S, double* u) {
  const double sigma = cms_det_log(S.s);
  double R[9];
  cms_s3o_quat_to_R(S.q, R);
  const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};      // deltaR
  const double eps = 0.00001;
  double A, B, C, om[3];
  if (fabs(sigma) < eps) {
    C = 1;
    if (d > 1 - eps) {
      for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
      A = 1. / 2.; B = 1. / 6.;
    } else {
      const double theta = cms_det_acos(d), theta2 = theta * theta;
      const double k = theta / (2 * sqrt(1 - d * d));
      for (int i = 0; i < 3; ++i) om[i] = k * dR[i];
      double sn, cs;
      cms_det_sincos(theta, &sn, &cs);
      A = (1 - cs) / theta2;
      B = (theta - sn) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (d > 1 - eps) {
      const double sigma2 = sigma * sigma;
      for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
      A = ((sigma - 1) * S.s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
    } else {
      const double theta = cms_det_acos(d);
      const double k = theta / (2 * sqrt(1 - d * d));
      for (int i = 0; i < 3; ++i) om[i] = k * dR[i];
      const double theta2 = theta * theta;
      double sn, cs;
      cms_det_sincos(theta, &sn, &cs);
      const double a = S.s * sn, b = S.s * cs, c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
    }
  }
  const double Om[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};      // skew
  double W[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {      // A*Omega + (B*Omega)*Omega + C*I
      const double bo2 = ((B * Om[3 * i]) * Om[j] + (B * Om[3 * i + 1]) * Om[3 + j]) + (B * Om[3 * i + 2]) * Om[6 + j];
      W[3 * i + j] = (A * Om[3 * i + j] + bo2) + C * (i == j ? 1.0 : 0.0);
    }
  cms_eg_lu3_solve(W, S.t, u + 3);
  u[0] = om[0]; u[1] = om[1]; u[2] = om[2];
  u[6] = sigma;
}

// Sji = Sjw * Swi, i = v0, j = v1 (:705-706, :753, :778, :809)
CMS_HD void cms_eg_measurement(const CmsS3& Siw, const CmsS3& Sjw, CmsS3* C) {
  CmsS3 Swi;
  cms_s3o_inverse(Siw, &Swi);
  cms_s3o_mul(Sjw, Swi, C);
}
// EdgeSim3::computeError: log(C * v0 * v1^-1)
CMS_HD void cms_eg_edge_error(const CmsS3& C, const CmsS3& S0, const CmsS3& S1, double* e) {
  CmsS3 a, inv1, b;
  cms_s3o_mul(C, S0, &a);
  cms_s3o_inverse(S1, &inv1);
  cms_s3o_mul(a, inv1, &b);
  cms_eg_log(b, e);
}
CMS_HD double cms_eg_chi(const double* e) {      // _error.dot(I * _error)
  double c = e[0] * e[0];
  for (int i = 1; i < 7; ++i) c = c + e[i] * e[i];
  return c;
}
// perturbed estimate k of linearizeOplus: oplus(+delta e_d) for k = 2 d, oplus(-delta e_d) for k = 2 d + 1
CMS_HD void cms_eg_perturb(const CmsS3& S, int fix_scale, int k, CmsS3* P) {
  double add[7] = {0, 0, 0, 0, 0, 0, 0};
  add[k >> 1] = (k & 1) ? -1e-9 : 1e-9;
  cms_s3o_oplus(S, add, fix_scale, P);
}
// column d of _jacobianOplusXi (which = 0) or Xj (which = 1), J 7 x 7 row major; Pv = the fourteen perturbed estimates of that vertex
CMS_HD void cms_eg_jac_column(const CmsS3& C, const CmsS3& S0, const CmsS3& S1, const CmsS3* Pv, int which, int d, double* J) {
  const double scalar = 1.0 / (2 * 1e-9);
  double ep[7], em[7];
  if (which == 0) { cms_eg_edge_error(C, Pv[2 * d], S1, ep); cms_eg_edge_error(C, Pv[2 * d + 1], S1, em); }
  else { cms_eg_edge_error(C, S0, Pv[2 * d], ep); cms_eg_edge_error(C, S0, Pv[2 * d + 1], em); }
  for (int r = 0; r < 7; ++r) J[7 * r + d] = scalar * (ep[r] - em[r]);
}

// ---- what one job works on.  The same record on the host (pointers into the host loop's vectors) and on the device (pointers into the handle's
// scratch): every phase below is a function of (work, task index) that the host loop calls for task 0, 1, ... and the kernel spreads over threads.
struct CmsEgOut { double chi2_initial, chi2_final, lambda_final; int iterations_run, trials_run, flags, pad; };
#define CMS_EG_FLAG_QMAX 1          // the last iteration ended on ten rejected trials
#define CMS_EG_FLAG_RHO0 2          // ... on rho == 0
#define CMS_EG_FLAG_NBAD 4          // ... on three iterations without progress
#define CMS_EG_FLAG_SOLVE 8         // some trial's factorisation met a zero or non-finite pivot
struct CmsEgWork {
  int N, fixed, E, fix_scale, iterations, Nf;
  double lambda_init;
  long long B;                      // envelope blocks
  const CmsS3* Scw; const CmsS3* Snc;
  const int* edges;                 // E x 3
  const int* inc_off; const int* inc;      // per vertex: its edges in ascending index (N + 1, 2 E)
  const int* first;                 // Nf
  const long long* rowp;            // Nf: block index of (i, first[i])
  const int* colp; const int* coli; // per pivot j: the rows i > j with first[i] <= j, ascending (Nf + 1, B - Nf)
  CmsS3 *S, *T, *P, *C;             // estimates, trial estimates (N each), perturbed estimates (14 N), measurements (E)
  double *err, *chi, *J;            // 7 E, E, 98 E
  double *H, *L;                    // 49 B each
  double *D, *RD, *b, *x, *sc;      // 7 Nf each, sc Nf
  CmsS3* S_out; float* Tiw_out; CmsEgOut* out;
};
CMS_HD int cms_eg_free_index(const CmsEgWork& w, int v) { return v - (v > w.fixed ? 1 : 0); }
CMS_HD int cms_eg_vertex(const CmsEgWork& w, int f) { return f + (f >= w.fixed ? 1 : 0); }
CMS_HD double* cms_eg_block(double* A, const CmsEgWork& w, int i, int j) { return A + 49 * (w.rowp[i] + (long long)(j - w.first[i])); }

CMS_HD void cms_eg_phase_measure(const CmsEgWork& w, int e) {
  const int v0 = w.edges[3 * e], v1 = w.edges[3 * e + 1];
  const CmsS3* M = w.edges[3 * e + 2] ? w.Snc : w.Scw;
  cms_eg_measurement(M[v0], M[v1], &w.C[e]);
}
CMS_HD void cms_eg_phase_perturb(const CmsEgWork& w, int t) {      // t in [0, 14 N)
  const int v = t / 14;
  if (v != w.fixed) cms_eg_perturb(w.S[v], w.fix_scale, t % 14, &w.P[t]);
}
CMS_HD void cms_eg_phase_error(const CmsEgWork& w, const CmsS3* est, int e) {
  double err[7];
  cms_eg_edge_error(w.C[e], est[w.edges[3 * e]], est[w.edges[3 * e + 1]], err);
  for (int i = 0; i < 7; ++i) w.err[7 * (size_t)e + i] = err[i];
  w.chi[e] = cms_eg_chi(err);
}
CMS_HD void cms_eg_phase_jacobian(const CmsEgWork& w, int t) {      // t in [0, 14 E): edge, vertex of the edge, column
  const int e = t / 14, which = (t % 14) / 7, d = t % 7;
  const int v = w.edges[3 * e + which];
  if (v == w.fixed) return;
  cms_eg_jac_column(w.C[e], w.S[w.edges[3 * e]], w.S[w.edges[3 * e + 1]], w.P + 14 * (size_t)v, which, d, w.J + 98 * (size_t)e + 49 * which);
}
// entry rc of free vertex f's row of blocks (H zeroed before): the diagonal block, the blocks left of it, and (rc % 7 == 0) entry rc / 7 of b
CMS_HD void cms_eg_phase_assemble(const CmsEgWork& w, int t) {      // t in [0, 49 Nf)
  const int f = t / 49, rc = t % 49, r = rc / 7, c = rc % 7;
  const int v = cms_eg_vertex(w, f);
  double diag = 0, bs = 0;
  for (int q = w.inc_off[v]; q < w.inc_off[v + 1]; ++q) {
    const int e = w.inc[q];
    const int side = w.edges[3 * e] == v ? 0 : 1, o = w.edges[3 * e + 1 - side];
    const double* Jv = w.J + 98 * (size_t)e + 49 * side;
    double dot = Jv[r] * Jv[c];
    for (int k = 1; k < 7; ++k) dot = dot + Jv[7 * k + r] * Jv[7 * k + c];
    diag = diag + dot;
    if (c == 0) {      // b += J^T (-(I e))
      const double* er = w.err + 7 * (size_t)e;
      double g = Jv[r] * (-er[0]);
      for (int k = 1; k < 7; ++k) g = g + Jv[7 * k + r] * (-er[k]);
      bs = bs + g;
    }
    if (o == w.fixed) continue;
    const int fo = cms_eg_free_index(w, o);
    if (fo > f) continue;
    const double* Jo = w.J + 98 * (size_t)e + 49 * (1 - side);
    double off = Jv[r] * Jo[c];
    for (int k = 1; k < 7; ++k) off = off + Jv[7 * k + r] * Jo[7 * k + c];
    double* blk = cms_eg_block(w.H, w, f, fo);
    blk[rc] = blk[rc] + off;
  }
  cms_eg_block(w.H, w, f, f)[rc] = diag;
  if (c == 0) w.b[7 * f + r] = bs;
}
CMS_HD void cms_eg_phase_damp(const CmsEgWork& w, double lambda, int t) {      // behind L = H; t in [0, 7 Nf)
  const int f = t / 7, r = t % 7;
  double* blk = cms_eg_block(w.L, w, f, f);
  blk[8 * r] = blk[8 * r] + lambda;
}
// the scalar LDL^T of cms_s3o_solve7 on one diagonal block, in place: unit lower triangle below the diagonal, D and 1 / D beside it
CMS_HD bool cms_eg_factor7(double* A, double* D, double* RD) {
  bool ok = true;
  for (int j = 0; j < 7; ++j) {
    double d = A[8 * j];
    for (int k = 0; k < j; ++k) d -= A[7 * j + k] * A[7 * j + k] * D[k];
    if (!(d - d == 0.0) || d == 0.0) ok = false;
    D[j] = d;
    const double rd = 1.0 / d;
    RD[j] = rd;
    for (int i = j + 1; i < 7; ++i) {
      double s = A[7 * i + j];
      for (int k = 0; k < j; ++k) s -= A[7 * i + k] * A[7 * j + k] * D[k];
      A[7 * i + j] = s * rd;
    }
  }
  return ok;
}
// row r of a block of column j: X <- X Ljj^-T D^-1, the same recurrence as cms_eg_factor7's rows below the diagonal
CMS_HD void cms_eg_scale_row(double* X, const double* Ljj, const double* D, const double* RD) {
  for (int c = 0; c < 7; ++c) {
    double s = X[c];
    for (int k = 0; k < c; ++k) s -= X[k] * Ljj[7 * c + k] * D[k];
    X[c] = s * RD[c];
  }
}
CMS_HD void cms_eg_phase_scale(const CmsEgWork& w, int j, const double* Ljj, const double* D, const double* RD, int t) {      // t in [0, 7 ncol)
  const int i = w.coli[w.colp[j] + t / 7];
  cms_eg_scale_row(cms_eg_block(w.L, w, i, j) + 7 * (t % 7), Ljj, D, RD);
}
// trailing update at pivot j: t in [0, 49 ncol^2); rows a >= b of column j's list, block (ia, ib) -= X(ia, j) D X(ib, j)^T
CMS_HD void cms_eg_phase_trail(const CmsEgWork& w, int j, const double* D, int ncol, long long t) {
  const int rc = (int)(t % 49), r = rc / 7, c = rc % 7;
  const int a = (int)(t / 49) / ncol, bq = (int)(t / 49) % ncol;
  if (bq > a) return;
  const int ia = w.coli[w.colp[j] + a], ib = w.coli[w.colp[j] + bq];
  const double* Xa = cms_eg_block(w.L, w, ia, j) + 7 * r;
  const double* Xb = cms_eg_block(w.L, w, ib, j) + 7 * c;
  double* dst = cms_eg_block(w.L, w, ia, ib) + rc;
  double s = *dst;
  for (int m = 0; m < 7; ++m) s -= Xa[m] * Xb[m] * D[m];
  *dst = s;
}
// forward substitution in x (= b on entry), row i: the blocks left of the diagonal (r in [0, 7)), then the unit triangle of the diagonal block
CMS_HD void cms_eg_phase_fwd_off(const CmsEgWork& w, int i, int r) {
  double s = w.x[7 * i + r];
  for (int j = w.first[i]; j < i; ++j) {
    const double* Lr = cms_eg_block(w.L, w, i, j) + 7 * r;
    for (int m = 0; m < 7; ++m) s -= Lr[m] * w.x[7 * j + m];
  }
  w.x[7 * i + r] = s;
}
CMS_HD void cms_eg_phase_fwd_diag(const CmsEgWork& w, int i) {
  const double* A = cms_eg_block(w.L, w, i, i);
  double* x = w.x + 7 * i;
  for (int r = 0; r < 7; ++r)
    for (int k = 0; k < r; ++k) x[r] -= A[7 * r + k] * x[k];
}
// D^-1 between the two substitutions: t in [0, 7 Nf)
CMS_HD void cms_eg_phase_dscale(const CmsEgWork& w, int t) { w.x[t] *= w.RD[t]; }
// back substitution, row k from the last: the diagonal block's transposed triangle, then x_j -= L(k, j)^T x_k for the blocks of the row
CMS_HD void cms_eg_phase_back_diag(const CmsEgWork& w, int k) {
  const double* A = cms_eg_block(w.L, w, k, k);
  double* x = w.x + 7 * k;
  for (int r = 6; r >= 0; --r)
    for (int m = r + 1; m < 7; ++m) x[r] -= A[7 * m + r] * x[m];
}
CMS_HD void cms_eg_phase_back_off(const CmsEgWork& w, int k, int t) {      // t in [0, 7 (k - first[k]))
  const int j = w.first[k] + t / 7, c = t % 7;
  const double* Lb = cms_eg_block(w.L, w, k, j);
  double s = w.x[7 * j + c];
  for (int r = 0; r < 7; ++r) s -= Lb[7 * r + c] * w.x[7 * k + r];
  w.x[7 * j + c] = s;
}
// the trial estimate of free vertex f (oplusImpl zeroes x[6] in the solver's own vector under fix_scale) and its share of computeScale
CMS_HD void cms_eg_phase_trial(const CmsEgWork& w, double lambda, int f) {
  const int v = cms_eg_vertex(w, f);
  double* x = w.x + 7 * f;
  cms_s3o_oplus(w.S[v], x, w.fix_scale, &w.T[v]);
  double scale = 0;
  for (int j = 0; j < 7; ++j) scale += x[j] * (lambda * x[j] + w.b[7 * f + j]);
  w.sc[f] = scale;
}

// ---- the Levenberg scalars one lane owns: CmsS3oLM's lambda, ni, currentChi, iniChi, rho, scale, nBad, qmax, ok2 with cms_s3o_lm_judge and
// cms_s3o_lm_stop as they stand (their S / trial / H / b are not used here).  computeLambdaInit returns the user's lambda
CMS_HD void cms_eg_lm_begin(CmsS3oLM* m, double chi, int it, double lambda_init) {
  m->currentChi = chi; m->iniChi = chi;
  if (it == 0) { m->lambda = lambda_init; m->ni = 2; m->nBad = 0; }
  m->rho = 0; m->qmax = 0;
}
// the judge; *accepted = the trial estimates become the estimates.  true: another trial
CMS_HD bool cms_eg_lm_judge(CmsS3oLM* m, double chi, double scale, int ok2, bool* accepted) {
  m->ok2 = ok2; m->scale = scale;
  const double tempChi = ok2 ? chi : 1.7976931348623157e308;
  const bool again = cms_s3o_lm_judge(m, chi);
  *accepted = m->rho > 0 && (tempChi - tempChi == 0.0);      // the judge's own condition
  return again;
}
CMS_HD int cms_eg_stop_flags(const CmsS3oLM* m) {
  return (m->qmax == 10 ? CMS_EG_FLAG_QMAX : 0) | (m->rho == 0 ? CMS_EG_FLAG_RHO0 : 0) | (m->nBad >= 3 ? CMS_EG_FLAG_NBAD : 0);
}

// ---- afterwards: Tiw = [R | (1/s) t] narrowed once (:833-852), row major 3 x 4
CMS_HD void cms_eg_pose_out(const CmsS3& S, float* T) {
  double R[9];
  cms_s3o_quat_to_R(S.q, R);
  const double is = 1. / S.s;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)R[3 * i + j];
    T[4 * i + 3] = (float)(S.t[i] * is);
  }
}
CMS_HD void cms_eg_phase_out(const CmsEgWork& w, int v) {
  CmsS3 o;
  for (int i = 0; i < 4; ++i) o.q[i] = cms_s3o_canon(w.S[v].q[i]);
  for (int i = 0; i < 3; ++i) o.t[i] = cms_s3o_canon(w.S[v].t[i]);
  o.s = cms_s3o_canon(w.S[v].s);
  w.S_out[v] = o;
  cms_eg_pose_out(o, w.Tiw_out + 12 * (size_t)v);
}
// correctedSwr.map(Srw.map(P)) (:854-885, LoopClosing.cpp:470-500): float to double, S_old.map, inverse(S_new).map, narrowed once
CMS_HD void cms_eg_correct_point(const float* p, const CmsS3& S_old, const CmsS3& S_new, float* o) {
  const double X[3] = {(double)p[0], (double)p[1], (double)p[2]};
  double y[3], z[3];
  CmsS3 inv;
  cms_s3o_map(S_old, X, y);
  cms_s3o_inverse(S_new, &inv);
  cms_s3o_map(inv, y, z);
  o[0] = (float)z[0]; o[1] = (float)z[1]; o[2] = (float)z[2];
}

#endif
