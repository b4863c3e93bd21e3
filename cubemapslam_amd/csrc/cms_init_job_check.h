// cms_init_job_check.h -- what cms_init_two_view checks per job before anything is enqueued, and the number of matches N (mvMatches12.size(),
// Initializer.cpp:61-75).  Host code, shared by the C-ABI entry (cms_api_init.hip) and the host loop (host/init_host.cpp), so both refuse the same
// records.  The draw rule is that of the PnP and Sim3 checks (cms_ransac_job_check.h).  Needs cms_init_job (include/cubemapslam_hip.h) before it.
#ifndef CMS_INIT_JOB_CHECK_H
#define CMS_INIT_JOB_CHECK_H
#include "cms_ransac_job_check.h"
// frames: frame 2 comes from a resident frame row (cms_init_two_view_frames): keys2 / rays2 are not read
static inline int cms_init_check_job(const cms_init_job& q, int* N_out, bool frames = false) {
  if (q.n1 < 1 || q.n2 < 1 || q.iterations < 1 || q.iterations > (1 << 20) || q.n_draws < 0) return CMS_ERR_ARG;
  if (!q.keys1 || !q.rays1 || !q.matches12 || !q.draws || !q.p3d || !q.triangulated) return CMS_ERR_ARG;
  if (frames ? q.b < 0 : (!q.keys2 || !q.rays2)) return CMS_ERR_ARG;
  int N = 0;
  for (int i = 0; i < q.n1; ++i) {
    if (q.matches12[i] >= q.n2) return CMS_ERR_ARG;
    if (q.matches12[i] >= 0) ++N;
  }
  *N_out = N;
  if (N < 8) return CMS_ERR_ARG;      // the reference pops from an empty vAvailableIndices; Tracking never gets here below 100 matches
  return cms_ransac_check_draws(q.draws, q.n_draws, q.iterations, 8, N);
}

// What is left of ReconstructE (:305-375) once the four CheckRT passes are done, for both callers: the decision of cms_init_core.h on nGood[4] and the
// four selected cosines, then the winner's pose, points and flags into the record.  cand_p3d / cand_good: the four passes' vP3D (3*n1 floats each)
// and vbGood (n1 bytes each), one after the other.  best_iteration < 0: no hypothesis scored above 0, nothing was reconstructed.
static inline void cms_init_finish_job(cms_init_job& q, int best_iteration, float score, int n_inliers, const int* nGood, const float* cosines,
                                       const float* R1, const float* R2, const float* t, const float* cand_p3d, const uint8_t* cand_good) {
  const size_t n1 = (size_t)q.n1;
  q.status = 0; q.winner = -1; q.best_iteration = best_iteration; q.score = score; q.n_inliers = n_inliers;
  for (int k = 0; k < 9; ++k) q.R21[k] = 0.0f;
  for (int k = 0; k < 3; ++k) q.t21[k] = 0.0f;
  for (int h = 0; h < 4; ++h) { q.nGood[h] = 0; q.parallax[h] = 0.0f; }
  for (size_t i = 0; i < 3 * n1; ++i) q.p3d[i] = 0.0f;
  for (size_t i = 0; i < n1; ++i) q.triangulated[i] = 0;
  if (best_iteration < 0) return;
  for (int h = 0; h < 4; ++h) q.nGood[h] = nGood[h];
  const int win = cms_init_decide(nGood, cosines, n_inliers, q.parallax);
  q.winner = win;
  if (win < 0) return;
  q.status = 1;
  const float* R = (win & 1) ? R2 : R1;
  for (int k = 0; k < 9; ++k) q.R21[k] = R[k];
  for (int k = 0; k < 3; ++k) q.t21[k] = win >= 2 ? -t[k] : t[k];
  for (size_t i = 0; i < 3 * n1; ++i) q.p3d[i] = cand_p3d[(size_t)win * 3 * n1 + i];
  for (size_t i = 0; i < n1; ++i) q.triangulated[i] = cand_good[(size_t)win * n1 + i];
}

#endif
