// cms_api_sim3.hip -- host side of Sim3Solver (src/Sim3Solver.cpp): cms_sim3_ransac_parameters, the cms_sim3 handle and cms_sim3_iterate;
// included by cms_lib.hip behind cms_api_frames.hip (cms_ctx, cms_fail, HIPCHK, CmsBlock, CmsStage) and cms_sim3_kernels.hip.  All jobs of a
// call are ONE launch sequence on the handle's stream: one pinned block up (the handle's CmsStage), k_sim3_hypotheses, k_sim3_select, one
// pinned block back.  Everything that becomes a device index (draws, counts, offsets) is checked on the host before anything is enqueued
// (cms_sim3_job_check.h).  The handle base, the head of an entry and the staging of the draws are cms_api_ransac.h, shared with the PnP and
// two-view entries.
#include <cstring>
#include <vector>
#include "cms_sim3_job_check.h"

struct cms_sim3 : CmsRansacHandle {
  int max_corr = 0, max_hyp = 0;
};

extern "C" int cms_sim3_ransac_parameters(int N, double probability, int minInliers, int maxIterations, int* max_its) {
  if (N < 0 || !max_its) return cms_fail(CMS_ERR_ARG, "cms_sim3_ransac_parameters: bad argument");
  const float epsilon = (float)minInliers / N;
  const int nIterations = minInliers == N ? 1 : cms_ransac_iterations(probability, epsilon);
  *max_its = std::max(1, std::min(nIterations, maxIterations));
  return CMS_OK;
}

extern "C" int cms_sim3_create(cms_sim3** out, int device, int max_jobs, int max_corr_total, int max_hyp_total) {
  if (!out || max_jobs < 1 || max_corr_total < 1 || max_hyp_total < 1) return cms_fail(CMS_ERR_ARG, "cms_sim3_create: bad argument");
  const int rcd = cms_check_device(device, "cms_sim3_create: no HIP device (the Sim3 solver's device path has no CPU fallback)");
  if (rcd) return rcd;
  cms_sim3* p = new cms_sim3();
  p->max_corr = max_corr_total; p->max_hyp = max_hyp_total;
  const int rc = p->open(device, max_jobs, true, "cms_sim3_create");
  if (rc) { cms_ransac_free(p); return rc; }
  *out = p;
  return CMS_OK;
}
extern "C" void cms_sim3_destroy(cms_sim3* p) { cms_ransac_free(p); }

extern "C" int cms_sim3_iterate(cms_sim3* p, cms_ctx* c, int njobs, cms_sim3_job* jobs) {
  int rc = cms_ransac_check_entry(p, c, njobs, jobs, "cms_sim3_iterate");
  if (rc || njobs == 0) return rc;
  std::vector<CmsSim3JobDev> jd((size_t)njobs);
  long long corr = 0, hyp = 0, words = 0, mwords = 0;
  for (int j = 0; j < njobs; ++j) {
    int H = 0, R = 0;
    rc = cms_sim3_check_job(jobs[j], &H, &R);
    if (rc) return cms_fail(rc, "cms_sim3_iterate: bad job (null array, draw outside [0, N-1-k], fewer than 3*H draws, best_mask against best_inliers, or a parameter out of range)");
    const cms_sim3_job& q = jobs[j];
    CmsSim3JobDev& d = jd[(size_t)j];
    d.N = q.N; d.H = R; d.corr0 = (int)corr; d.hyp0 = (int)hyp; d.words = (q.N + 63) / 64; d.word0 = words; d.mword0 = (int)mwords;
    d.fix_scale = q.fix_scale ? 1 : 0; d.min_inliers = q.min_inliers; d.max_its = q.max_its; d.iterations = q.iterations; d.best_inliers = q.best_inliers;
    std::memcpy(d.best, q.best_R, 36); std::memcpy(d.best + 9, q.best_t, 12); d.best[12] = q.best_s; std::memcpy(d.best + 13, q.best_T12, 48);
    corr += q.N; hyp += R; words += (long long)R * d.words; mwords += d.words;
    if (corr > p->max_corr) return cms_fail(CMS_ERR_ARG, "cms_sim3_iterate: more correspondences than the handle was created for");
    if (hyp > p->max_hyp) return cms_fail(CMS_ERR_ARG, "cms_sim3_iterate: more hypotheses than the handle was created for");
  }
  const size_t C_ = (size_t)corr, Hn = (size_t)hyp, J_ = (size_t)njobs, MW = (size_t)mwords;
  CmsBlock blk;
  const size_t o_jobs = blk.take(J_ * sizeof(CmsSim3JobDev)), o_hjob = blk.take(Hn * 4), o_draws = blk.take(Hn * 12), o_x1 = blk.take(C_ * 12), o_x2 = blk.take(C_ * 12),
               o_me1 = blk.take(C_ * 4), o_me2 = blk.take(C_ * 4), o_bin = blk.take(MW * 8);
  const size_t in_bytes = blk.size;
  const size_t o_out = blk.take(J_ * sizeof(CmsSim3OutDev)), o_bout = blk.take(MW * 8);
  const size_t out_begin = o_out, out_end = blk.size;
  const size_t o_mot = blk.take(Hn * 100), o_cnt = blk.take(Hn * 4), o_hmask = blk.take((size_t)words * 8);
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  rc = p->blocks.reserve(s, blk.size, out_end);
  if (rc) return rc;
  uint8_t* h = p->blocks.h;
  uint8_t* d = p->blocks.d;
  std::memset(h, 0, in_bytes);
  std::memcpy(h + o_jobs, jd.data(), J_ * sizeof(CmsSim3JobDev));
  for (int j = 0; j < njobs; ++j) {
    const cms_sim3_job& q = jobs[j];
    const CmsSim3JobDev& g = jd[(size_t)j];
    cms_ransac_stage_draws<3>(reinterpret_cast<int*>(h + o_hjob) + g.hyp0, reinterpret_cast<int*>(h + o_draws) + 3 * (size_t)g.hyp0, j, g.H, q.draws);
    if (q.N == 0) continue;
    const size_t c0 = (size_t)g.corr0, n = (size_t)q.N;
    std::memcpy(h + o_x1 + 12 * c0, q.x3dc1, 12 * n); std::memcpy(h + o_x2 + 12 * c0, q.x3dc2, 12 * n);
    std::memcpy(h + o_me1 + 4 * c0, q.max_err1, 4 * n); std::memcpy(h + o_me2 + 4 * c0, q.max_err2, 4 * n);
    cms_mask_pack(q.best_mask, q.N, reinterpret_cast<unsigned long long*>(h + o_bin) + g.mword0);
  }
  rc = p->blocks.up(s, in_bytes, "cms_sim3_iterate");
  if (rc) return rc;
  CmsSim3Args a = {};
  a.F = c->g.F; a.njobs = njobs; a.nhyp = (int)hyp;
  a.jobs = (const CmsSim3JobDev*)(d + o_jobs); a.hyp_job = (const int*)(d + o_hjob); a.draws = (const int*)(d + o_draws);
  a.x1 = (const float*)(d + o_x1); a.x2 = (const float*)(d + o_x2); a.me1 = (const float*)(d + o_me1); a.me2 = (const float*)(d + o_me2);
  a.hyp_motion = (float*)(d + o_mot); a.hyp_count = (int*)(d + o_cnt); a.hyp_mask = (unsigned long long*)(d + o_hmask);
  a.best_in = (const unsigned long long*)(d + o_bin); a.best_out = (unsigned long long*)(d + o_bout); a.out = (CmsSim3OutDev*)(d + o_out);
  if (hyp > 0) {
    hipLaunchKernelGGL(k_sim3_hypotheses, dim3((int)hyp), dim3(64), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_sim3_select, dim3(njobs), dim3(64), 0, s, a);
  HIPCHK(hipGetLastError());
  rc = p->blocks.back_and_wait(s, out_begin, out_end, "cms_sim3_iterate");
  if (rc) return rc;
  for (int j = 0; j < njobs; ++j) {
    cms_sim3_job& q = jobs[j];
    const CmsSim3JobDev& g = jd[(size_t)j];
    q.status = 0; q.no_more = 0; q.n_inliers = 0; q.iterations_run = 0;
    std::memset(q.T12, 0, sizeof(q.T12));
    if (q.N > 0) std::memset(q.inliers, 0, (size_t)q.N);
    if (q.N < q.min_inliers) { q.no_more = 1; continue; }      // :170-174, nothing else is touched
    const CmsSim3OutDev& o = reinterpret_cast<const CmsSim3OutDev*>(h + o_out)[j];
    const unsigned long long* bo = reinterpret_cast<const unsigned long long*>(h + o_bout) + g.mword0;
    q.iterations = o.iterations; q.iterations_run = o.iterations_run; q.best_inliers = o.best_inliers; q.no_more = o.no_more; q.status = o.status;
    std::memcpy(q.best_R, o.best, 36); std::memcpy(q.best_t, o.best + 9, 12); q.best_s = o.best[12]; std::memcpy(q.best_T12, o.best + 13, 48);
    cms_mask_unpack(bo, q.N, q.best_mask);
    if (o.status == 1) {
      q.n_inliers = o.n_inliers;
      std::memcpy(q.T12, q.best_T12, sizeof(q.T12));
      std::memcpy(q.inliers, q.best_mask, (size_t)q.N);
    }
  }
  return CMS_OK;
}
