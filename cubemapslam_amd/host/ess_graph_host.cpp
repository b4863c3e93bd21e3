// ess_graph_host.cpp -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:623-886) on the CPU over the job records of
// cms_essential_graph_optimize: the literal sequence, one task after the other, through the host build of csrc/cms_ess_graph_core.h.  This is the
// definition of record the device entry is held to bit for bit (tests/test_gpu_essential_graph.py), and the stage probes the CPU tests compare
// with the numpy restatement.
#include <cstdio>
#include <cstring>
#include <vector>
#include "cubemapslam_hip.h"
#include "../csrc/cms_ess_graph_core.h"
#include "../csrc/cms_ess_graph_job_check.h"

namespace {
thread_local const char* g_why = "";
thread_local char g_msg[160];

// the slots of one sum, folded by the core's tree: item k adds into slot k mod 256 in ascending k
double slot_sum(const double* v, int n) {
  double s[CMS_SIM3_OPT_SLOTS];
  for (int i = 0; i < CMS_SIM3_OPT_SLOTS; ++i) s[i] = 0;
  for (int k = 0; k < n; ++k) s[k % CMS_SIM3_OPT_SLOTS] += v[k];
  return cms_s3o_tree(s);
}

// the factorisation of L (= H + lambda I on entry) and the solve into x; false on a zero / non-finite pivot
bool solve(const CmsEgWork& w) {
  bool ok = true;
  for (int j = 0; j < w.Nf; ++j) {
    double* Ljj = cms_eg_block(w.L, w, j, j);
    if (!cms_eg_factor7(Ljj, w.D + 7 * j, w.RD + 7 * j)) ok = false;
    const int ncol = w.colp[j + 1] - w.colp[j];
    for (int t = 0; t < 7 * ncol; ++t) cms_eg_phase_scale(w, j, Ljj, w.D + 7 * j, w.RD + 7 * j, t);
    for (long long t = 0; t < 49LL * ncol * ncol; ++t) cms_eg_phase_trail(w, j, w.D + 7 * j, ncol, t);
  }
  for (int i = 0; i < 7 * w.Nf; ++i) w.x[i] = w.b[i];
  for (int i = 0; i < w.Nf; ++i) {
    for (int r = 0; r < 7; ++r) cms_eg_phase_fwd_off(w, i, r);
    cms_eg_phase_fwd_diag(w, i);
  }
  for (int t = 0; t < 7 * w.Nf; ++t) cms_eg_phase_dscale(w, t);
  for (int k = w.Nf - 1; k >= 0; --k) {
    cms_eg_phase_back_diag(w, k);
    for (int t = 0; t < 7 * (k - w.first[k]); ++t) cms_eg_phase_back_off(w, k, t);
  }
  return ok;
}

double errors_at(const CmsEgWork& w, const CmsS3* est) {
  for (int e = 0; e < w.E; ++e) cms_eg_phase_error(w, est, e);
  return slot_sum(w.chi, w.E);
}

void optimize_one(cms_ess_graph_job& q) {
  const int N = q.N, E = q.E, Nf = N - 1;
  CmsEgStructure st;
  cms_eg_structure(N, q.fixed, E, q.edges, st);
  const size_t B = (size_t)st.blocks;
  std::vector<CmsS3> S((size_t)N), T((size_t)N), P(14 * (size_t)N), C((size_t)E), So((size_t)N);
  std::vector<double> err(7 * (size_t)E), chi((size_t)E), J(98 * (size_t)E), H(49 * B), L(49 * B), D(7 * (size_t)Nf), RD(7 * (size_t)Nf), b(7 * (size_t)Nf), x(7 * (size_t)Nf),
      sc((size_t)Nf);
  std::memcpy(S.data(), q.Scw, sizeof(CmsS3) * (size_t)N);
  T = S;
  CmsEgOut out = {};
  CmsEgWork w = {};
  w.N = N; w.fixed = q.fixed; w.E = E; w.fix_scale = q.fix_scale ? 1 : 0; w.iterations = q.iterations; w.Nf = Nf; w.lambda_init = q.lambda_init; w.B = st.blocks;
  w.Scw = reinterpret_cast<const CmsS3*>(q.Scw); w.Snc = reinterpret_cast<const CmsS3*>(q.Snc); w.edges = q.edges;
  w.inc_off = st.inc_off.data(); w.inc = st.inc.data(); w.first = st.first.data(); w.rowp = st.rowp.data(); w.colp = st.colp.data(); w.coli = st.coli.data();
  w.S = S.data(); w.T = T.data(); w.P = P.data(); w.C = C.data(); w.err = err.data(); w.chi = chi.data(); w.J = J.data(); w.H = H.data(); w.L = L.data();
  w.D = D.data(); w.RD = RD.data(); w.b = b.data(); w.x = x.data(); w.sc = sc.data();
  w.S_out = So.data(); w.Tiw_out = q.Tiw_out; w.out = &out;

  for (int e = 0; e < E; ++e) cms_eg_phase_measure(w, e);
  CmsS3oLM lm;
  std::memset(&lm, 0, sizeof(lm));
  lm.lambda = q.lambda_init; lm.ni = 2; lm.fix_scale = w.fix_scale;
  const double chi0 = errors_at(w, w.S);
  lm.currentChi = chi0;
  int done = 0, trials = 0, flags = 0;
  for (int it = 0; it < q.iterations && Nf > 0 && E > 0; ++it) {
    for (int t = 0; t < 14 * N; ++t) cms_eg_phase_perturb(w, t);
    const double c = errors_at(w, w.S);
    for (int t = 0; t < 14 * E; ++t) cms_eg_phase_jacobian(w, t);
    for (size_t i = 0; i < 49 * B; ++i) H[i] = 0;
    for (int t = 0; t < 49 * Nf; ++t) cms_eg_phase_assemble(w, t);
    cms_eg_lm_begin(&lm, c, it, q.lambda_init);
    for (;;) {
      for (size_t i = 0; i < 49 * B; ++i) L[i] = H[i];
      for (int t = 0; t < 7 * Nf; ++t) cms_eg_phase_damp(w, lm.lambda, t);
      const int ok2 = solve(w) ? 1 : 0;
      if (!ok2) { flags |= CMS_EG_FLAG_SOLVE; for (int i = 0; i < 7 * Nf; ++i) x[(size_t)i] = 0; }
      for (int f = 0; f < Nf; ++f) cms_eg_phase_trial(w, lm.lambda, f);
      const double scale = slot_sum(w.sc, Nf);
      const double tc = errors_at(w, w.T);
      bool accepted;
      const bool again = cms_eg_lm_judge(&lm, tc, scale, ok2, &accepted);
      ++trials;
      if (accepted) for (int v = 0; v < N; ++v) if (v != w.fixed) S[(size_t)v] = T[(size_t)v];
      if (!again) break;
    }
    ++done;
    if (cms_s3o_lm_stop(&lm)) { flags |= cms_eg_stop_flags(&lm); break; }
  }
  for (int v = 0; v < N; ++v) cms_eg_phase_out(w, v);
  std::memcpy(q.S_out, So.data(), sizeof(CmsS3) * (size_t)N);
  q.chi2_initial = cms_s3o_canon(chi0); q.chi2_final = cms_s3o_canon(lm.currentChi); q.lambda_final = cms_s3o_canon(lm.lambda);
  q.iterations_run = done; q.trials_run = trials; q.flags = flags;
}

const char* check_call(int njobs, const cms_ess_graph_job* jobs, int max_jobs, int max_vertices, int max_edges, long long max_blocks, int* rc) {
  *rc = CMS_ERR_ARG;
  if (njobs < 0 || (njobs > 0 && !jobs)) return "bad argument";
  if (njobs > max_jobs) return "more jobs than the handle was created for";
  long long V = 0, E = 0, B = 0;
  std::vector<int> first;
  for (int j = 0; j < njobs; ++j) {
    const char* why = cms_ess_graph_check_job(jobs[j]);
    if (why) return why;
    V += jobs[j].N; E += jobs[j].E;
    if (V > max_vertices) return "more vertices than the handle was created for";
    if (E > max_edges) return "more edges than the handle was created for";
    B += cms_eg_envelope(jobs[j].N, jobs[j].fixed, jobs[j].E, jobs[j].edges, first);
  }
  if (B > max_blocks) {
    *rc = CMS_ERR_OVERFLOW;
    snprintf(g_msg, sizeof(g_msg), "the jobs' envelopes need %lld blocks, the handle has %lld", B, max_blocks);
    return g_msg;
  }
  *rc = CMS_OK;
  return nullptr;
}
}  // namespace

extern "C" const char* hm_ess_graph_last_reason() { return g_why; }

// the entry's checks against a handle of the given capacities: CMS_OK, CMS_ERR_ARG or CMS_ERR_OVERFLOW, the reason in hm_ess_graph_last_reason
extern "C" int hm_ess_graph_job_check(int njobs, const cms_ess_graph_job* jobs, int max_jobs, int max_vertices, int max_edges, int max_blocks) {
  int rc;
  const char* why = check_call(njobs, jobs, max_jobs, max_vertices, max_edges, max_blocks, &rc);
  g_why = why ? why : "";
  return rc;
}

extern "C" int hm_essential_graph_optimize_host(int njobs, cms_ess_graph_job* jobs) {
  int rc;
  const char* why = check_call(njobs, jobs, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffffffffffffLL, &rc);
  g_why = why ? why : "";
  if (rc) return rc;
  for (int j = 0; j < njobs; ++j) optimize_one(jobs[j]);
  return CMS_OK;
}

extern "C" int hm_sim3_correct_points_host(int n, const float* pos_in, const int* ref, int K, const double* S_old, const double* S_new, float* pos_out) {
  g_why = "";
  if (n < 0 || K < 0 || (n > 0 && (!pos_in || !ref || !pos_out))) { g_why = "bad argument"; return CMS_ERR_ARG; }
  for (int k = 0; k < n; ++k)
    if (ref[k] >= K || (ref[k] >= 0 && (!S_old || !S_new))) { g_why = "ref out of range"; return CMS_ERR_ARG; }
  for (int k = 0; k < n; ++k) {
    if (ref[k] < 0) { for (int i = 0; i < 3; ++i) pos_out[3 * k + i] = pos_in[3 * k + i]; continue; }
    cms_eg_correct_point(pos_in + 3 * k, reinterpret_cast<const CmsS3*>(S_old)[ref[k]], reinterpret_cast<const CmsS3*>(S_new)[ref[k]], pos_out + 3 * k);
  }
  return CMS_OK;
}

// ---- stage probes (tests)
extern "C" double hm_det_log(double x) { return cms_det_log(x); }
extern "C" double hm_det_acos(double x) { return cms_det_acos(x); }
extern "C" void hm_eg_log(const double* S8, double* u7) { CmsS3 S; std::memcpy(&S, S8, sizeof(S)); cms_eg_log(S, u7); }
// the error of one edge: measurement from (Mi, Mj) = the operand set's entries of v0 / v1, estimates S0 / S1
extern "C" void hm_eg_edge_error(const double* Mi, const double* Mj, const double* S0, const double* S1, double* e7) {
  CmsS3 a, b, s0, s1, C;
  std::memcpy(&a, Mi, 64); std::memcpy(&b, Mj, 64); std::memcpy(&s0, S0, 64); std::memcpy(&s1, S1, 64);
  cms_eg_measurement(a, b, &C);
  cms_eg_edge_error(C, s0, s1, e7);
}
// both numeric Jacobians (7 x 7 row major) of one edge with both vertices free
extern "C" void hm_eg_edge_jacobians(const double* Mi, const double* Mj, const double* S0, const double* S1, int fix_scale, double* J0, double* J1) {
  CmsS3 a, b, s0, s1, C, P0[14], P1[14];
  std::memcpy(&a, Mi, 64); std::memcpy(&b, Mj, 64); std::memcpy(&s0, S0, 64); std::memcpy(&s1, S1, 64);
  cms_eg_measurement(a, b, &C);
  for (int k = 0; k < 14; ++k) { cms_eg_perturb(s0, fix_scale, k, &P0[k]); cms_eg_perturb(s1, fix_scale, k, &P1[k]); }
  for (int d = 0; d < 7; ++d) { cms_eg_jac_column(C, s0, s1, P0, 0, d, J0); cms_eg_jac_column(C, s0, s1, P1, 1, d, J1); }
}
// first (N - 1 ints) and the block count of a job's envelope
extern "C" long long hm_eg_envelope(int N, int fixed, int E, const int* edges, int* first) {
  std::vector<int> f;
  const long long B = cms_eg_envelope(N, fixed, E, edges, f);
  if (first) for (size_t i = 0; i < f.size(); ++i) first[i] = f[i];
  return B;
}
// (H + lambda I) x = b through the core's envelope factorisation, H given dense (n = 7 Nf, row major; entries outside the envelope are not read);
// the graph (N, fixed, E, edges) names the envelope.  Returns 1, or 0 on a zero / non-finite pivot
extern "C" int hm_eg_envelope_solve(int N, int fixed, int E, const int* edges, const double* Hd, const double* bv, double lambda, double* xv) {
  CmsEgStructure st;
  cms_eg_structure(N, fixed, E, edges, st);
  const int Nf = N - 1, n = 7 * Nf;
  std::vector<double> L(49 * (size_t)st.blocks), D((size_t)n), RD((size_t)n), b(bv, bv + n), x((size_t)n);
  CmsEgWork w = {};
  w.N = N; w.fixed = fixed; w.E = E; w.Nf = Nf; w.B = st.blocks; w.edges = edges;
  w.first = st.first.data(); w.rowp = st.rowp.data(); w.colp = st.colp.data(); w.coli = st.coli.data();
  w.L = L.data(); w.D = D.data(); w.RD = RD.data(); w.b = b.data(); w.x = x.data();
  for (int i = 0; i < Nf; ++i)
    for (int j = st.first[(size_t)i]; j <= i; ++j) {
      double* blk = cms_eg_block(w.L, w, i, j);
      for (int r = 0; r < 7; ++r)
        for (int c = 0; c < 7; ++c) blk[7 * r + c] = Hd[(size_t)(7 * i + r) * n + 7 * j + c];
    }
  for (int t = 0; t < n; ++t) cms_eg_phase_damp(w, lambda, t);
  const bool ok = solve(w);
  for (int i = 0; i < n; ++i) xv[i] = x[(size_t)i];
  return ok ? 1 : 0;
}
