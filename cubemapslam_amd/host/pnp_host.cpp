// pnp_host.cpp -- PnPsolver::iterate (src/PnPsolver.cpp:167-261) on the CPU over the job records of cms_pnp_iterate: the literal loop, one hypothesis
// after the other, through the host build of csrc/cms_pnp_core.h.  This is the definition of record the device entry is held to bit for bit
// (tests/test_gpu_pnp.py), and the stage dumps the CPU tests compare with the numpy restatement.
#include <cstring>
#include <vector>
#include "cubemapslam_hip.h"
#include "../csrc/cms_pnp_core.h"
#include "../csrc/cms_pnp_job_check.h"

namespace {
struct HostSolver {
  const cms_pnp_job& q;
  int F;
  std::vector<float> max_error;
  std::vector<double> pws, us, bearings, alphas, pcs;
  int number_of_correspondences = 0;
  double mRi[9], mti[3];
  std::vector<uint8_t> inliersi;
  int nInliersi = 0;
  HostSolver(const cms_pnp_job& job, int F_) : q(job), F(F_), max_error((size_t)job.N), inliersi((size_t)job.N, 0) {
    for (int i = 0; i < q.N; ++i) max_error[(size_t)i] = q.sigma2[i] * q.th2;
    std::memset(mRi, 0, sizeof(mRi)); std::memset(mti, 0, sizeof(mti));
  }
  void reset(int n) { number_of_correspondences = 0; pws.resize(3 * (size_t)n); us.resize(2 * (size_t)n); bearings.resize(3 * (size_t)n); alphas.resize(4 * (size_t)n); pcs.resize(3 * (size_t)n); }
  void add(int idx) {      // add_bearing_correspondence (:369-383)
    const size_t k = (size_t)number_of_correspondences++;
    for (int j = 0; j < 3; ++j) { pws[3 * k + j] = q.p3d[3 * idx + j]; bearings[3 * k + j] = static_cast<double>(q.bearing[3 * idx + j]); }
    us[2 * k] = q.p2d[2 * idx]; us[2 * k + 1] = q.p2d[2 * idx + 1];
  }
  void compute_pose() {
    double mtm[144], ut[144];
    cms_pnp_compute_pose(number_of_correspondences, F, pws.data(), us.data(), bearings.data(), alphas.data(), pcs.data(), mtm, ut, mRi, mti, nullptr);
  }
  void check_inliers() {
    nInliersi = 0;
    for (int i = 0; i < q.N; ++i) {
      const bool in = cms_pnp_is_inlier(F, mRi, mti, q.p3d + 3 * i, q.p2d + 2 * i, max_error[(size_t)i]);
      inliersi[(size_t)i] = in ? 1 : 0;
      if (in) nInliersi++;
    }
  }
  void tcw(float* T) const { for (int i = 0; i < 9; ++i) T[i] = (float)mRi[i]; for (int i = 0; i < 3; ++i) T[9 + i] = (float)mti[i]; }
};

void iterate_one(int F, cms_pnp_job& q) {
  q.status = 0; q.no_more = 0; q.n_inliers = 0; q.iterations_run = 0;
  std::memset(q.Tcw, 0, sizeof(q.Tcw));
  if (q.N > 0) std::memset(q.inliers, 0, (size_t)q.N);
  if (q.N < q.min_inliers) { q.no_more = 1; return; }
  HostSolver S(q, F);
  std::vector<size_t> vAllIndices((size_t)q.N), vAvailableIndices;
  for (int i = 0; i < q.N; ++i) vAllIndices[(size_t)i] = (size_t)i;
  const int* draw = q.draws;
  int nCurrentIterations = 0;
  while (q.iterations < q.max_its || nCurrentIterations < q.n_iterations) {
    nCurrentIterations++;
    q.iterations++;
    S.reset(4);
    vAvailableIndices = vAllIndices;
    for (short i = 0; i < 4; ++i) {
      const int randi = *draw++;
      const int idx = (int)vAvailableIndices[(size_t)randi];
      S.add(idx);
      vAvailableIndices[(size_t)randi] = vAvailableIndices.back();
      vAvailableIndices.pop_back();
    }
    S.compute_pose();
    S.check_inliers();
    if (S.nInliersi >= q.min_inliers) {
      if (S.nInliersi > q.best_inliers) {
        std::memcpy(q.best_mask, S.inliersi.data(), (size_t)q.N);
        q.best_inliers = S.nInliersi;
        S.tcw(q.best_Tcw);
      }
      // Refine (:263-309)
      std::vector<int> vIndices;
      for (int i = 0; i < q.N; ++i)
        if (q.best_mask[i]) vIndices.push_back(i);
      S.reset((int)vIndices.size());
      for (size_t i = 0; i < vIndices.size(); ++i) S.add(vIndices[i]);
      S.compute_pose();
      S.check_inliers();
      if (S.nInliersi > q.min_inliers) {
        q.status = 1; q.n_inliers = S.nInliersi; q.iterations_run = nCurrentIterations;
        S.tcw(q.Tcw);
        std::memcpy(q.inliers, S.inliersi.data(), (size_t)q.N);
        return;
      }
    }
  }
  q.iterations_run = nCurrentIterations;
  if (q.iterations >= q.max_its) {
    q.no_more = 1;
    if (q.best_inliers >= q.min_inliers) {
      q.status = 2; q.n_inliers = q.best_inliers;
      std::memcpy(q.Tcw, q.best_Tcw, sizeof(q.Tcw));
      std::memcpy(q.inliers, q.best_mask, (size_t)q.N);
    }
  }
}
}  // namespace

extern "C" int hm_pnp_iterate_host(int F, int njobs, cms_pnp_job* jobs) {
  if (F <= 0 || njobs < 0 || (njobs > 0 && !jobs)) return CMS_ERR_ARG;
  for (int j = 0; j < njobs; ++j) {
    int H = 0;
    const int rc = cms_pnp_check_job(jobs[j], &H);
    if (rc) return rc;
  }
  for (int j = 0; j < njobs; ++j) iterate_one(F, jobs[j]);
  return CMS_OK;
}

// One EPnP solve on the listed correspondences with every stage handed out (tests): idx[n] into the job's arrays; ut 144, R 9, t 3
extern "C" int hm_pnp_compute_pose(int F, const cms_pnp_job* job, int n, const int* idx, CmsPnpStages* st, double* ut, double* alphas, double* R, double* t, double* rep) {
  if (!job || n < 1 || !idx) return CMS_ERR_ARG;
  HostSolver S(*job, F);
  S.reset(n);
  for (int i = 0; i < n; ++i) {
    if (idx[i] < 0 || idx[i] >= job->N) return CMS_ERR_ARG;
    S.add(idx[i]);
  }
  double mtm[144];
  const double e = cms_pnp_compute_pose(n, F, S.pws.data(), S.us.data(), S.bearings.data(), S.alphas.data(), S.pcs.data(), mtm, ut, R, t, st);
  if (alphas) std::memcpy(alphas, S.alphas.data(), sizeof(double) * 4 * (size_t)n);
  if (rep) *rep = e;
  return CMS_OK;
}
// CheckInliers over N correspondences for a pose of the caller's; returns the count
extern "C" int hm_pnp_check_inliers(int F, int N, const double* R, const double* t, const float* p3d, const float* p2d, const float* max_error, uint8_t* out) {
  int c = 0;
  for (int i = 0; i < N; ++i) { out[i] = cms_pnp_is_inlier(F, R, t, p3d + 3 * i, p2d + 2 * i, max_error[i]) ? 1 : 0; c += out[i]; }
  return c;
}
extern "C" void hm_pnp_jacobi(int m, int n, double* At, double* Vt, double* w) { cms_pnp_jacobi(m, n, At, Vt, w); }
extern "C" void hm_pnp_resolve_draws(int N, const int* draws, int* idx) { cms_pnp_resolve_draws(N, draws, idx); }
extern "C" int hm_pnp_stages_size() { return (int)sizeof(CmsPnpStages); }
