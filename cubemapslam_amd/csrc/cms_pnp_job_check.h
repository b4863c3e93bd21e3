// cms_pnp_job_check.h -- what cms_pnp_iterate checks per job before anything is enqueued, and the number of hypotheses H the call may need
// (PnPsolver.cpp:175, :184).  Host code, shared by the C-ABI entry (cms_api_pnp.hip) and the host loop (host/pnp_host.cpp), so both refuse the
// same records.  The rules it shares with the Sim3 and two-view checks are cms_ransac_job_check.h.  Needs cms_pnp_job (include/cubemapslam_hip.h)
// before it.
#ifndef CMS_PNP_JOB_CHECK_H
#define CMS_PNP_JOB_CHECK_H
#include "cms_ransac_job_check.h"
// frames: the 2-D side comes from a resident frame row (cms_pnp_iterate_frames): kp_idx instead of p2d / bearing / sigma2
static inline int cms_pnp_check_job(const cms_pnp_job& q, int* H_out, bool frames = false) {
  // SetRansacParameters never gives min_inliers below minSet = 4 (Refine on an empty best mask would divide by zero)
  if (cms_ransac_check_counters(q, 4)) return CMS_ERR_ARG;
  if (q.min_set != 4) return CMS_ERR_UNSUPPORTED;
  int H = 0, H_min = 0;
  cms_ransac_hypotheses(q.N, q.min_inliers, q.max_its, q.iterations, q.n_iterations, &H, &H_min);
  *H_out = H;      // PnP runs H_max: `while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations)` (:184)
  if (q.N > 0 && (!q.p3d || !q.best_mask || !q.inliers)) return CMS_ERR_ARG;
  if (q.N > 0 && (frames ? !q.kp_idx : (!q.p2d || !q.bearing || !q.sigma2))) return CMS_ERR_ARG;
  if (frames) {
    if (q.b < 0 || q.n < 0) return CMS_ERR_ARG;
    for (int i = 0; i < q.N; ++i)
      if (q.kp_idx[i] < 0 || q.kp_idx[i] >= q.n) return CMS_ERR_ARG;
  }
  if (cms_ransac_check_draws(q.draws, q.n_draws, H, 4, q.N)) return CMS_ERR_ARG;
  return cms_ransac_check_best_mask(q.best_mask, q.N, q.best_inliers);
}

#endif
