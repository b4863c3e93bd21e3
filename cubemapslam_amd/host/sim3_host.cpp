// sim3_host.cpp -- Sim3Solver::iterate (src/Sim3Solver.cpp:164-231) on the CPU over the job records of cms_sim3_iterate: the literal loop, one
// hypothesis after the other, through the host build of csrc/cms_sim3_core.h.  This is the definition of record the device entry is held to bit
// for bit (tests/test_gpu_sim3.py), and the stage dumps the CPU tests compare with the numpy restatement.
#include <cstring>
#include <vector>
#include "cubemapslam_hip.h"
#include "../csrc/cms_sim3_core.h"
#include "../csrc/cms_sim3_job_check.h"

namespace {
void iterate_one(int F, cms_sim3_job& q) {
  q.status = 0; q.no_more = 0; q.n_inliers = 0; q.iterations_run = 0;
  std::memset(q.T12, 0, sizeof(q.T12));
  if (q.N > 0) std::memset(q.inliers, 0, (size_t)q.N);
  if (q.N < q.min_inliers) { q.no_more = 1; return; }      // :170-174
  std::vector<size_t> vAllIndices((size_t)q.N), vAvailableIndices;
  for (int i = 0; i < q.N; ++i) vAllIndices[(size_t)i] = (size_t)i;
  std::vector<uint8_t> vbInliersi((size_t)q.N, 0);
  const int* draw = q.draws;
  float P3Dc1i[9], P3Dc2i[9];      // point k at [3k..3k+2]
  CmsSim3Motion m;
  int nCurrentIterations = 0;
  while (q.iterations < q.max_its && nCurrentIterations < q.n_iterations) {
    nCurrentIterations++;
    q.iterations++;
    vAvailableIndices = vAllIndices;
    for (short i = 0; i < 3; ++i) {
      const int randi = *draw++;
      const int idx = (int)vAvailableIndices[(size_t)randi];
      for (int c = 0; c < 3; ++c) { P3Dc1i[3 * i + c] = q.x3dc1[3 * idx + c]; P3Dc2i[3 * i + c] = q.x3dc2[3 * idx + c]; }
      vAvailableIndices[(size_t)randi] = vAvailableIndices.back();
      vAvailableIndices.pop_back();
    }
    cms_sim3_compute(P3Dc1i, P3Dc2i, q.fix_scale, &m, nullptr);
    int nInliersi = 0;
    for (int i = 0; i < q.N; ++i) {
      const bool in = cms_sim3_is_inlier(F, m.T12, m.T21, q.x3dc1 + 3 * i, q.x3dc2 + 3 * i, q.max_err1[i], q.max_err2[i]);
      vbInliersi[(size_t)i] = in ? 1 : 0;
      if (in) nInliersi++;
    }
    if (nInliersi >= q.best_inliers) {
      std::memcpy(q.best_mask, vbInliersi.data(), (size_t)q.N);
      q.best_inliers = nInliersi;
      std::memcpy(q.best_T12, m.T12, sizeof(q.best_T12));
      std::memcpy(q.best_R, m.R, sizeof(q.best_R));
      std::memcpy(q.best_t, m.t, sizeof(q.best_t));
      q.best_s = m.s;
      if (nInliersi > q.min_inliers) {
        q.status = 1; q.n_inliers = nInliersi; q.iterations_run = nCurrentIterations;
        std::memcpy(q.T12, q.best_T12, sizeof(q.T12));
        std::memcpy(q.inliers, vbInliersi.data(), (size_t)q.N);
        return;
      }
    }
  }
  q.iterations_run = nCurrentIterations;
  if (q.iterations >= q.max_its) q.no_more = 1;
}
}  // namespace

extern "C" int hm_sim3_iterate_host(int F, int njobs, cms_sim3_job* jobs) {
  if (F <= 0 || njobs < 0 || (njobs > 0 && !jobs)) return CMS_ERR_ARG;
  for (int j = 0; j < njobs; ++j) {
    int H = 0, R = 0;
    const int rc = cms_sim3_check_job(jobs[j], &H, &R);
    if (rc) return rc;
  }
  for (int j = 0; j < njobs; ++j) iterate_one(F, jobs[j]);
  return CMS_OK;
}

// One ComputeSim3 on three pairs (P1, P2: point k at [3k..3k+2]) with every intermediate handed out (tests)
extern "C" void hm_sim3_compute(const float* P1, const float* P2, int fix_scale, CmsSim3Motion* m, CmsSim3Stages* st) { cms_sim3_compute(P1, P2, fix_scale, m, st); }
// CheckInliers over N correspondences for a motion of the caller's; returns the count
extern "C" int hm_sim3_check_inliers(int F, int N, const float* T12, const float* T21, const float* x1, const float* x2, const float* me1, const float* me2, uint8_t* out) {
  int c = 0;
  for (int i = 0; i < N; ++i) { out[i] = cms_sim3_is_inlier(F, T12, T21, x1 + 3 * i, x2 + 3 * i, me1[i], me2[i]) ? 1 : 0; c += out[i]; }
  return c;
}
extern "C" int hm_sim3_jacobi4(double* A, double* V) { return cms_sim3_jacobi4(A, V); }
extern "C" void hm_sim3_quat_to_R(const float* q, float* R) { cms_sim3_quat_to_R(q, R); }
extern "C" void hm_sim3_resolve_draws(int N, const int* draws, int* idx) { cms_sim3_resolve_draws(N, draws, idx); }
extern "C" int hm_sim3_stages_size() { return (int)sizeof(CmsSim3Stages); }
extern "C" int hm_sim3_motion_size() { return (int)sizeof(CmsSim3Motion); }
