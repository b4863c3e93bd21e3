// cms_sim3_job_check.h -- what cms_sim3_iterate checks per job before anything is enqueued.  Host code, shared by the C-ABI entry
// (cms_api_sim3.hip) and the host loop (host/sim3_host.cpp), so both refuse the same records.  Needs cms_sim3_job (include/cubemapslam_hip.h)
// before it.
//   H_draws  the iterations the caller has to bring draws for: max(max_its - iterations, n_iterations), 0 when N < min_inliers
//   H_run    the hypotheses a call can evaluate: the `while (mnIterations < max_its && nCurrentIterations < n_iterations)` of Sim3Solver.cpp:182
//            runs min(max_its - iterations, n_iterations) times unless a hypothesis is accepted before
#ifndef CMS_SIM3_JOB_CHECK_H
#define CMS_SIM3_JOB_CHECK_H
static inline int cms_sim3_check_job(const cms_sim3_job& q, int* H_draws, int* H_run) {
  // three pairs make a hypothesis; the counters stay far from int's end
  if (q.min_inliers < 3 || q.max_its < 0 || q.max_its > (1 << 20) || q.n_iterations < 0 || q.n_iterations > (1 << 20) || q.iterations > (1 << 30)) return CMS_ERR_ARG;
  if (q.N < 0 || q.n_draws < 0 || q.iterations < 0 || q.best_inliers < 0 || q.best_inliers > q.N) return CMS_ERR_ARG;
  int H = 0, R = 0;
  if (q.N >= q.min_inliers) {
    const int left = q.max_its - q.iterations;
    H = left > q.n_iterations ? left : q.n_iterations;
    R = left < q.n_iterations ? left : q.n_iterations;
    if (H < 0) H = 0;
    if (R < 0) R = 0;
  }
  *H_draws = H; *H_run = R;
  if (q.N > 0 && (!q.x3dc1 || !q.x3dc2 || !q.max_err1 || !q.max_err2 || !q.best_mask || !q.inliers)) return CMS_ERR_ARG;
  if (H > 0 && ((long long)q.n_draws < 3LL * H || !q.draws)) return CMS_ERR_ARG;
  for (int i = 0; i < H; ++i)
    for (int k = 0; k < 3; ++k)
      if (q.draws[3 * i + k] < 0 || q.draws[3 * i + k] > q.N - 1 - k) return CMS_ERR_ARG;
  int nb = 0;
  for (int i = 0; i < q.N; ++i) nb += q.best_mask[i] ? 1 : 0;
  if (nb != q.best_inliers) return CMS_ERR_ARG;
  return CMS_OK;
}

#endif
