// cms_pnp_job_check.h -- what cms_pnp_iterate checks per job before anything is enqueued, and the number of hypotheses H the call may need
// (PnPsolver.cpp:175, :184).  Host code, shared by the C-ABI entry (cms_api_pnp.hip) and the host loop (host/pnp_host.cpp), so both refuse the
// same records.  Needs cms_pnp_job (include/cubemapslam_hip.h) before it.
#ifndef CMS_PNP_JOB_CHECK_H
#define CMS_PNP_JOB_CHECK_H
// frames: the 2-D side comes from a resident frame row (cms_pnp_iterate_frames): kp_idx instead of p2d / bearing / sigma2
static inline int cms_pnp_check_job(const cms_pnp_job& q, int* H_out, bool frames = false) {
  // SetRansacParameters never gives min_inliers below minSet = 4 (Refine on an empty best mask would divide by zero); the counters stay far from int's end
  if (q.min_inliers < 4 || q.max_its < 0 || q.max_its > (1 << 20) || q.n_iterations < 0 || q.n_iterations > (1 << 20) || q.iterations > (1 << 30)) return CMS_ERR_ARG;
  if (q.N < 0 || q.n_draws < 0 || q.iterations < 0 || q.best_inliers < 0 || q.best_inliers > q.N) return CMS_ERR_ARG;
  if (q.min_set != 4) return CMS_ERR_UNSUPPORTED;
  int H = 0;
  if (q.N >= q.min_inliers) {
    H = q.max_its - q.iterations;
    if (H < q.n_iterations) H = q.n_iterations;
    if (H < 0) H = 0;
  }
  *H_out = H;
  if (q.N > 0 && (!q.p3d || !q.best_mask || !q.inliers)) return CMS_ERR_ARG;
  if (q.N > 0 && (frames ? !q.kp_idx : (!q.p2d || !q.bearing || !q.sigma2))) return CMS_ERR_ARG;
  if (frames) {
    if (q.b < 0 || q.n < 0) return CMS_ERR_ARG;
    for (int i = 0; i < q.N; ++i)
      if (q.kp_idx[i] < 0 || q.kp_idx[i] >= q.n) return CMS_ERR_ARG;
  }
  if (H > 0 && ((long long)q.n_draws < 4LL * H || !q.draws)) return CMS_ERR_ARG;
  for (int i = 0; i < H; ++i)
    for (int k = 0; k < 4; ++k)
      if (q.draws[4 * i + k] < 0 || q.draws[4 * i + k] > q.N - 1 - k) return CMS_ERR_ARG;
  int nb = 0;
  for (int i = 0; i < q.N; ++i) nb += q.best_mask[i] ? 1 : 0;
  if (nb != q.best_inliers) return CMS_ERR_ARG;
  return CMS_OK;
}

#endif
