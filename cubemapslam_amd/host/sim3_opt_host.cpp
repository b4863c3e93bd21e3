// sim3_opt_host.cpp -- Optimizer::OptimizeSim3 (src/Optimizer.cpp:888-1091) on the CPU over the job records of cms_sim3_optimize: the literal
// sequence, one pair after the other, through the host build of csrc/cms_sim3_opt_core.h.  This is the definition of record the device entry is
// held to bit for bit (tests/test_gpu_sim3_opt.py), and the stage probes the CPU tests compare with the numpy restatement.
#include <cstring>
#include <vector>
#include "cubemapslam_hip.h"
#include "../csrc/cms_sim3_opt_core.h"
#include "../csrc/cms_sim3_opt_job_check.h"

namespace {
struct Graph {
  int F, mode, fix_scale;
  double delta;
  std::vector<CmsS3oPair> pairs;
  std::vector<uint8_t> active;       // the pair's edges are still in the graph
  std::vector<double> err;           // 4 per pair: the persistent _error of e12 | e21
};

// the slots of one pass, folded by the core's tree
double fold(std::vector<double>& slots, int width, int which) {
  double s[CMS_SIM3_OPT_SLOTS];
  for (int i = 0; i < CMS_SIM3_OPT_SLOTS; ++i) s[i] = slots[(size_t)i * width + which];
  return cms_s3o_tree(s);
}

// computeActiveErrors + buildSystem at L.S: sum[36]
void linearise(Graph& g, const CmsS3oLin& L, double* sum) {
  std::vector<double> slots((size_t)CMS_SIM3_OPT_SLOTS * CMS_SIM3_OPT_ACC, 0.0);
  for (size_t k = 0; k < g.pairs.size(); ++k) {
    if (!g.active[k]) continue;
    const CmsS3oPair& p = g.pairs[k];
    double* e = &g.err[4 * k];
    double J12[14], J21[14];
    cms_s3o_errors(g.F, p, L.S, L.Sinv, e);
    cms_s3o_pair_jac(g.F, g.mode, g.fix_scale, p, L, J12, J21);      // the numeric Jacobian restores _error afterwards: e stays
    double* acc = &slots[(k % CMS_SIM3_OPT_SLOTS) * CMS_SIM3_OPT_ACC];
    cms_s3o_edge_accumulate(J12, e, p.om1, g.delta, acc);
    cms_s3o_edge_accumulate(J21, e + 2, p.om2, g.delta, acc);
  }
  for (int i = 0; i < CMS_SIM3_OPT_ACC; ++i) sum[i] = fold(slots, CMS_SIM3_OPT_ACC, i);
}

// computeActiveErrors + activeRobustChi2 at S
double trial_chi(Graph& g, const CmsS3& S) {
  CmsS3 Sinv;
  cms_s3o_inverse(S, &Sinv);
  std::vector<double> slots((size_t)CMS_SIM3_OPT_SLOTS, 0.0);
  for (size_t k = 0; k < g.pairs.size(); ++k) {
    if (!g.active[k]) continue;
    double* e = &g.err[4 * k];
    cms_s3o_errors(g.F, g.pairs[k], S, Sinv, e);
    cms_s3o_pair_chi(g.pairs[k], e, g.delta, &slots[k % CMS_SIM3_OPT_SLOTS]);
  }
  return fold(slots, 1, 0);
}

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg; returns the iterations run
int optimize(Graph& g, CmsS3oLM& lm, int iterations) {
  int done = 0;
  for (int it = 0; it < iterations; ++it) {
    CmsS3oLin L;
    cms_s3o_lin_base(lm.S, &L);
    if (g.mode == CMS_SIM3_OPT_AS_WRITTEN)
      for (int k = 0; k < 14; ++k) cms_s3o_lin_perturb(lm.S, g.fix_scale, k, &L);
    double sum[CMS_SIM3_OPT_ACC];
    linearise(g, L, sum);
    cms_s3o_lm_begin(&lm, sum, it);
    for (;;) {
      cms_s3o_lm_trial(&lm);
      if (!cms_s3o_lm_judge(&lm, trial_chi(g, lm.trial))) break;
    }
    ++done;
    if (cms_s3o_lm_stop(&lm)) break;
  }
  return done;
}

int classify(Graph& g, float th2, uint8_t* keep) {
  int bad = 0;
  for (size_t k = 0; k < g.pairs.size(); ++k) {
    if (!g.active[k]) continue;
    if (cms_s3o_pair_is_bad(g.pairs[k], &g.err[4 * k], th2)) { keep[k] = 0; g.active[k] = 0; ++bad; }
  }
  return bad;
}

void put(cms_sim3_opt_job& q, const CmsS3& S) {
  for (int i = 0; i < 4; ++i) q.q12[i] = cms_s3o_canon(S.q[i]);
  for (int i = 0; i < 3; ++i) q.t12_out[i] = cms_s3o_canon(S.t[i]);
  q.s12_out = cms_s3o_canon(S.s);
}

void optimize_one(int F, cms_sim3_opt_job& q) {
  Graph g;
  g.F = F; g.mode = q.jacobian; g.fix_scale = q.fix_scale ? 1 : 0; g.delta = cms_s3o_huber_delta(q.th2);
  g.pairs.resize((size_t)q.N); g.active.assign((size_t)q.N, 1); g.err.assign(4 * (size_t)q.N, 0.0);
  for (int k = 0; k < q.N; ++k) {
    cms_s3o_pair_setup(F, q.x3dc1 + 3 * k, q.x3dc2 + 3 * k, q.kp1 + 2 * k, q.kp2 + 2 * k, q.inv_sigma2_1[k], q.inv_sigma2_2[k], &g.pairs[(size_t)k]);
    q.keep[k] = 1;
  }
  CmsS3 S0;
  cms_s3o_from_Rts(q.R12, q.t12, q.s12, &S0);
  CmsS3oLM lm;
  std::memset(&lm, 0, sizeof(lm));
  lm.S = S0; lm.trial = S0; lm.fix_scale = g.fix_scale;
  q.n_correspondences = q.N; q.n_inliers = 0; q.n_bad = 0; q.iterations[0] = 0; q.iterations[1] = 0;
  if (q.N > 0) q.iterations[0] = optimize(g, lm, 5);      // no edge: no active vertex, optimize() returns at once
  const int nBad = classify(g, q.th2, q.keep);
  q.n_bad = nBad;
  if (q.N - nBad < 10) { put(q, S0); return; }           // :1061, g2oS12 untouched
  q.iterations[1] = optimize(g, lm, cms_s3o_more_iterations(nBad));
  const int bad2 = classify(g, q.th2, q.keep);
  q.n_inliers = q.N - nBad - bad2;
  put(q, lm.S);
}

thread_local const char* g_why = "";
}  // namespace

extern "C" const char* hm_sim3_opt_last_reason() { return g_why; }

extern "C" int hm_sim3_optimize_host(int F, int njobs, cms_sim3_opt_job* jobs) {
  g_why = "";
  if (F <= 0 || njobs < 0 || (njobs > 0 && !jobs)) { g_why = "bad argument"; return CMS_ERR_ARG; }
  for (int j = 0; j < njobs; ++j) {
    const char* why = cms_sim3_opt_check_job(F, jobs[j]);
    if (why) { g_why = why; return CMS_ERR_ARG; }
  }
  for (int j = 0; j < njobs; ++j) optimize_one(F, jobs[j]);
  return CMS_OK;
}

// ---- stage probes (tests)
extern "C" double hm_s3o_exp(double x) { return cms_det_exp(x); }
extern "C" void hm_s3o_sincos(double x, double* s, double* c) { cms_det_sincos(x, s, c); }
// Sim3(Vector7d) -> q xyzw | t | s
extern "C" void hm_s3o_sim3_exp(const double* u, double* out8) { CmsS3 S; cms_s3o_exp(u, &S); std::memcpy(out8, &S, sizeof(S)); }
extern "C" void hm_s3o_R_to_quat(const double* R, double* q) { cms_s3o_R_to_quat(R, q); }
extern "C" void hm_s3o_oplus(const double* S8, double* u, int fix_scale, double* out8) {
  CmsS3 S, O; std::memcpy(&S, S8, sizeof(S)); cms_s3o_oplus(S, u, fix_scale, &O); std::memcpy(out8, &O, sizeof(O));
}
extern "C" void hm_s3o_inverse(const double* S8, double* out8) { CmsS3 S, O; std::memcpy(&S, S8, sizeof(S)); cms_s3o_inverse(S, &O); std::memcpy(out8, &O, sizeof(O)); }
// both edges' errors (e12 | e21) of one correspondence at S; returns 0, or -1 when a key point lies in no face
extern "C" int hm_s3o_edge_errors(int F, const double* S8, const float* x1, const float* x2, const float* kp1, const float* kp2, double* e4) {
  CmsS3 S, Sinv; std::memcpy(&S, S8, sizeof(S));
  CmsS3oPair p;
  if (!cms_s3o_pair_setup(F, x1, x2, kp1, kp2, 1.0f, 1.0f, &p)) return -1;
  cms_s3o_inverse(S, &Sinv);
  cms_s3o_errors(F, p, S, Sinv, e4);
  return 0;
}
// both edges' Jacobians (2 x 7 row major each) of one correspondence at S in either mode
extern "C" int hm_s3o_edge_jacobians(int F, int mode, int fix_scale, const double* S8, const float* x1, const float* x2, const float* kp1, const float* kp2, double* J12,
                                     double* J21) {
  CmsS3 S; std::memcpy(&S, S8, sizeof(S));
  CmsS3oPair p;
  if (!cms_s3o_pair_setup(F, x1, x2, kp1, kp2, 1.0f, 1.0f, &p)) return -1;
  CmsS3oLin L;
  cms_s3o_lin_base(S, &L);
  for (int k = 0; k < 14; ++k) cms_s3o_lin_perturb(S, fix_scale, k, &L);
  cms_s3o_pair_jac(F, mode, fix_scale, p, L, J12, J21);
  return 0;
}
extern "C" int hm_s3o_solve7(const double* H, const double* b, double lambda, double* x) { return cms_s3o_solve7(H, b, lambda, x) ? 1 : 0; }
extern "C" double hm_s3o_tree(const double* slots) {
  double s[CMS_SIM3_OPT_SLOTS];
  std::memcpy(s, slots, sizeof(s));
  return cms_s3o_tree(s);
}
extern "C" int hm_s3o_slots() { return CMS_SIM3_OPT_SLOTS; }
