// cms_api_pnp.hip -- host side of PnPsolver (src/PnPsolver.cpp): cms_pnp_ransac_parameters, the cms_pnp handle, cms_pnp_iterate and
// cms_pnp_iterate_frames (k_pnp_gather in front, the context's stream instead of the handle's); included by
// cms_lib.hip behind cms_api_frames.hip (cms_ctx, cms_fail, HIPCHK, CmsBlock) and cms_pnp_kernels.hip.  All jobs of a call are ONE launch
// sequence on the handle's stream: one pinned block up (the handle's CmsStage), k_pnp_hypotheses, k_pnp_inliers, k_pnp_select, one pinned block back.  Everything that
// becomes a device index (draws, counts, offsets) is checked on the host before anything is enqueued (cms_pnp_job_check.h).  The handle base, the
// head of an entry and the staging of the draws are cms_api_ransac.h, shared with the Sim3 and two-view entries.
#include <cstring>
#include <vector>
#include "cms_pnp_job_check.h"

struct cms_pnp : CmsRansacHandle {
  int max_corr = 0, max_hyp = 0;
};

extern "C" int cms_pnp_ransac_parameters(int N, double probability, int minInliers, int maxIterations, int minSet, float epsilon, int* min_inliers,
                                         int* max_its, float* epsilon_out) {
  if (N < 0 || !min_inliers || !max_its) return cms_fail(CMS_ERR_ARG, "cms_pnp_ransac_parameters: bad argument");
  float mRansacEpsilon = epsilon;
  int nMinInliers = (int)(N * mRansacEpsilon);
  if (nMinInliers < minInliers) nMinInliers = minInliers;
  if (nMinInliers < minSet) nMinInliers = minSet;
  if (mRansacEpsilon < (float)nMinInliers / N) mRansacEpsilon = (float)nMinInliers / N;
  const int nIterations = nMinInliers == N ? 1 : cms_ransac_iterations(probability, mRansacEpsilon);
  *min_inliers = nMinInliers;
  *max_its = std::max(1, std::min(nIterations, maxIterations));
  if (epsilon_out) *epsilon_out = mRansacEpsilon;
  return CMS_OK;
}

extern "C" int cms_pnp_create(cms_pnp** out, int device, int max_jobs, int max_corr_total, int max_hyp_total) {
  if (!out || max_jobs < 1 || max_corr_total < 1 || max_hyp_total < 1) return cms_fail(CMS_ERR_ARG, "cms_pnp_create: bad argument");
  const int rcd = cms_check_device(device, "cms_pnp_create: no HIP device (the PnP solver's device path has no CPU fallback)");
  if (rcd) return rcd;
  cms_pnp* p = new cms_pnp();
  p->max_corr = max_corr_total; p->max_hyp = max_hyp_total;
  const int rc = p->open(device, max_jobs, true, "cms_pnp_create");
  if (rc) { cms_ransac_free(p); return rc; }
  *out = p;
  return CMS_OK;
}
extern "C" void cms_pnp_destroy(cms_pnp* p) { cms_ransac_free(p); }

// frames: cms_pnp_iterate_frames -- the 2-D side is gathered on the device from the context's resident rows, and the whole sequence runs on the
// context's stream (behind whatever filled the rows), as cms_kfstore_search_by_projection does
static int cms_pnp_run(cms_pnp* p, cms_ctx* c, int njobs, cms_pnp_job* jobs, bool frames) {
  int rc = cms_ransac_check_entry(p, c, njobs, jobs, "cms_pnp_iterate");
  if (rc || njobs == 0) return rc;
  std::vector<CmsPnpJobDev> jd((size_t)njobs);
  long long corr = 0, hyp = 0, words = 0, mwords = 0;
  for (int j = 0; j < njobs; ++j) {
    int H = 0;
    rc = cms_pnp_check_job(jobs[j], &H, frames);
    if (rc == CMS_ERR_UNSUPPORTED) return cms_fail(rc, "cms_pnp_iterate: min_set must be 4 (Refine is the n-point path)");
    if (rc) return cms_fail(rc, "cms_pnp_iterate: bad job (null array, draw outside [0, N-1-k], fewer than 4*H draws, or best_mask against best_inliers)");
    const cms_pnp_job& q = jobs[j];
    if (frames && (q.b >= c->max_batch || q.n > c->g.kp_cap)) return cms_fail(CMS_ERR_ARG, "cms_pnp_iterate_frames: frame row or key-point count beyond the context's");
    CmsPnpJobDev& d = jd[(size_t)j];
    d.N = q.N; d.H = H; d.corr0 = (int)corr; d.hyp0 = (int)hyp; d.words = (q.N + 63) / 64; d.word0 = words; d.mword0 = (int)mwords;
    d.min_inliers = q.min_inliers; d.max_its = q.max_its; d.iterations = q.iterations; d.best_inliers = q.best_inliers;
    std::memcpy(d.best_Tcw, q.best_Tcw, sizeof(d.best_Tcw));
    corr += q.N; hyp += H; words += (long long)H * d.words; mwords += d.words;
    if (corr > p->max_corr) return cms_fail(CMS_ERR_ARG, "cms_pnp_iterate: more correspondences than the handle was created for");
    if (hyp > p->max_hyp) return cms_fail(CMS_ERR_ARG, "cms_pnp_iterate: more hypotheses than the handle was created for");
  }
  const size_t C_ = (size_t)corr, Hn = (size_t)hyp, J_ = (size_t)njobs, MW = (size_t)mwords;
  CmsBlock blk;
  const size_t o_jobs = blk.take(J_ * sizeof(CmsPnpJobDev)), o_hjob = blk.take(Hn * 4), o_draws = blk.take(Hn * 16), o_p3d = blk.take(C_ * 12), o_p2d = blk.take(C_ * 8),
               o_bear = blk.take(C_ * 12), o_maxe = blk.take(C_ * 4), o_bin = blk.take(MW * 8),
               o_cjob = blk.take(C_ * 4), o_kpi = blk.take(C_ * 4), o_jrow = blk.take(J_ * 4), o_jth2 = blk.take(J_ * 4);
  const size_t in_bytes = blk.size;
  const size_t o_out = blk.take(J_ * sizeof(CmsPnpOutDev)), o_bout = blk.take(MW * 8), o_rout = blk.take(MW * 8);
  const size_t out_begin = o_out, out_end = blk.size;
  const size_t o_rt = blk.take(Hn * 96), o_cnt = blk.take(Hn * 4), o_hmask = blk.take((size_t)words * 8), o_rows = blk.take(C_ * 15 * 8);
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = frames ? c->stream : p->stream;
  rc = p->blocks.reserve(s, blk.size, out_end);
  if (rc) return rc;
  uint8_t* h = p->blocks.h;
  uint8_t* d = p->blocks.d;
  std::memset(h, 0, in_bytes);
  std::memcpy(h + o_jobs, jd.data(), J_ * sizeof(CmsPnpJobDev));
  for (int j = 0; j < njobs; ++j) {
    const cms_pnp_job& q = jobs[j];
    const CmsPnpJobDev& g = jd[(size_t)j];
    cms_ransac_stage_draws<4>(reinterpret_cast<int*>(h + o_hjob) + g.hyp0, reinterpret_cast<int*>(h + o_draws) + 4 * (size_t)g.hyp0, j, g.H, q.draws);
    if (q.N == 0) continue;
    const size_t c0 = (size_t)g.corr0, n = (size_t)q.N;
    std::memcpy(h + o_p3d + 12 * c0, q.p3d, 12 * n);
    if (frames) {
      std::memcpy(h + o_kpi + 4 * c0, q.kp_idx, 4 * n);
      int* cj = reinterpret_cast<int*>(h + o_cjob) + c0;
      for (size_t i = 0; i < n; ++i) cj[i] = j;
      reinterpret_cast<int*>(h + o_jrow)[j] = q.b; reinterpret_cast<float*>(h + o_jth2)[j] = q.th2;
    } else {
      std::memcpy(h + o_p2d + 8 * c0, q.p2d, 8 * n); std::memcpy(h + o_bear + 12 * c0, q.bearing, 12 * n);
      float* me = reinterpret_cast<float*>(h + o_maxe) + c0;
      for (size_t i = 0; i < n; ++i) me[i] = q.sigma2[i] * q.th2;      // mvMaxError[i] = mvSigma2[i]*th2 (:158), float
    }
    cms_mask_pack(q.best_mask, q.N, reinterpret_cast<unsigned long long*>(h + o_bin) + g.mword0);
  }
  rc = p->blocks.up(s, in_bytes, "cms_pnp_iterate");
  if (rc) return rc;
  if (frames && corr > 0) {
    CmsPnpGatherArgs ga = {};
    ga.ncorr = (int)corr; ga.kp_cap = c->g.kp_cap; ga.nlevels = c->g.nlevels;
    ga.corr_job = (const int*)(d + o_cjob); ga.job_row = (const int*)(d + o_jrow); ga.job_th2 = (const float*)(d + o_jth2); ga.kp_idx = (const int*)(d + o_kpi);
    ga.kps = (const CmsKeyPoint*)c->d_kps; ga.rays = c->d_rays;
    cms_level_table(ga.sigma2, c, c->sigma2, 1.0f);
    ga.p2d = (float*)(d + o_p2d); ga.bearing = (float*)(d + o_bear); ga.max_error = (float*)(d + o_maxe);
    hipLaunchKernelGGL(k_pnp_gather, dim3(((int)corr + 255) / 256), dim3(256), 0, s, ga);
    HIPCHK(hipGetLastError());
  }
  CmsPnpArgs a = {};
  a.F = c->g.F; a.njobs = njobs; a.nhyp = (int)hyp;
  a.jobs = (const CmsPnpJobDev*)(d + o_jobs); a.hyp_job = (const int*)(d + o_hjob); a.draws = (const int*)(d + o_draws);
  a.p3d = (const float*)(d + o_p3d); a.p2d = (const float*)(d + o_p2d); a.bearing = (const float*)(d + o_bear); a.max_error = (const float*)(d + o_maxe);
  a.hyp_Rt = (double*)(d + o_rt); a.hyp_count = (int*)(d + o_cnt); a.hyp_mask = (unsigned long long*)(d + o_hmask);
  a.best_in = (const unsigned long long*)(d + o_bin); a.best_out = (unsigned long long*)(d + o_bout); a.refined_out = (unsigned long long*)(d + o_rout);
  a.refine_rows = (double*)(d + o_rows); a.out = (CmsPnpOutDev*)(d + o_out);
  if (hyp > 0) {
    static bool lds_done[64] = {};
    const int lds = CMS_PNP_HYP_LANES * CMS_PNP_LANE_DOUBLES * (int)sizeof(double);
    rc = cms_lds_ceiling_once((const void*)k_pnp_hypotheses, lds, p->device, lds_done);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3(((int)hyp + CMS_PNP_HYP_LANES - 1) / CMS_PNP_HYP_LANES), dim3(CMS_PNP_HYP_LANES), lds, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_inliers, dim3((int)hyp), dim3(64), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_pnp_select, dim3(njobs), dim3(CMS_PNP_SELECT_THREADS), 0, s, a);
  HIPCHK(hipGetLastError());
  rc = p->blocks.back_and_wait(s, out_begin, out_end, "cms_pnp_iterate");
  if (rc) return rc;
  for (int j = 0; j < njobs; ++j) {
    cms_pnp_job& q = jobs[j];
    const CmsPnpJobDev& g = jd[(size_t)j];
    q.status = 0; q.no_more = 0; q.n_inliers = 0; q.iterations_run = 0;
    std::memset(q.Tcw, 0, sizeof(q.Tcw));
    if (q.N > 0) std::memset(q.inliers, 0, (size_t)q.N);
    if (q.N < q.min_inliers) { q.no_more = 1; continue; }      // :175-179, nothing else is touched
    const CmsPnpOutDev& o = reinterpret_cast<const CmsPnpOutDev*>(h + o_out)[j];
    const unsigned long long* bo = reinterpret_cast<const unsigned long long*>(h + o_bout) + g.mword0;
    const unsigned long long* ro = reinterpret_cast<const unsigned long long*>(h + o_rout) + g.mword0;
    q.iterations = o.iterations; q.iterations_run = o.iterations_run; q.best_inliers = o.best_inliers; q.no_more = o.no_more; q.status = o.status;
    std::memcpy(q.best_Tcw, o.best_Tcw, sizeof(q.best_Tcw));
    cms_mask_unpack(bo, q.N, q.best_mask);
    if (o.status == 1) {
      q.n_inliers = o.n_inliers;
      std::memcpy(q.Tcw, o.Tcw, sizeof(q.Tcw));
      cms_mask_unpack(ro, q.N, q.inliers);
    } else if (o.status == 2) {
      q.n_inliers = q.best_inliers;
      std::memcpy(q.Tcw, q.best_Tcw, sizeof(q.Tcw));
      std::memcpy(q.inliers, q.best_mask, (size_t)q.N);
    }
  }
  return CMS_OK;
}

extern "C" int cms_pnp_iterate(cms_pnp* p, cms_ctx* c, int njobs, cms_pnp_job* jobs) { return cms_pnp_run(p, c, njobs, jobs, false); }
extern "C" int cms_pnp_iterate_frames(cms_pnp* p, cms_ctx* c, int njobs, cms_pnp_job* jobs) { return cms_pnp_run(p, c, njobs, jobs, true); }
