// cms_sim3_job_check.h -- what cms_sim3_iterate checks per job before anything is enqueued.  Host code, shared by the C-ABI entry
// (cms_api_sim3.hip) and the host loop (host/sim3_host.cpp), so both refuse the same records.  Needs cms_sim3_job (include/cubemapslam_hip.h)
// before it.  The rules it shares with the PnP and two-view checks are cms_ransac_job_check.h.
//   H_draws  the iterations the caller has to bring draws for: max(max_its - iterations, n_iterations), 0 when N < min_inliers
//   H_run    the hypotheses a call can evaluate: the `while (mnIterations < max_its && nCurrentIterations < n_iterations)` of Sim3Solver.cpp:182
//            runs min(max_its - iterations, n_iterations) times unless a hypothesis is accepted before
#ifndef CMS_SIM3_JOB_CHECK_H
#define CMS_SIM3_JOB_CHECK_H
#include "cms_ransac_job_check.h"
static inline int cms_sim3_check_job(const cms_sim3_job& q, int* H_draws, int* H_run) {
  if (cms_ransac_check_counters(q, 3)) return CMS_ERR_ARG;      // three pairs make a hypothesis
  // Sim3 brings draws for H_max and runs H_min: `while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations)` (:182)
  cms_ransac_hypotheses(q.N, q.min_inliers, q.max_its, q.iterations, q.n_iterations, H_draws, H_run);
  if (q.N > 0 && (!q.x3dc1 || !q.x3dc2 || !q.max_err1 || !q.max_err2 || !q.best_mask || !q.inliers)) return CMS_ERR_ARG;
  if (cms_ransac_check_draws(q.draws, q.n_draws, *H_draws, 3, q.N)) return CMS_ERR_ARG;
  return cms_ransac_check_best_mask(q.best_mask, q.N, q.best_inliers);
}

#endif
