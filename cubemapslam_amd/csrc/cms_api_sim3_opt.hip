// cms_api_sim3_opt.hip -- host side of Optimizer::OptimizeSim3 (src/Optimizer.cpp:888-1091): the cms_sim3_opt handle and cms_sim3_optimize;
// included by cms_lib.hip behind cms_api_frames.hip (cms_ctx, cms_fail, HIPCHK, CmsBlock, CmsStage), cms_api_ransac.h (the handle base and the
// check at the head of an entry, which the solver entries share) and cms_sim3_opt_kernels.hip.  All jobs of a call are ONE launch sequence on
// the handle's stream: one pinned block up (the handle's CmsStage), k_sim3_optimize, one pinned block back.  Everything that becomes a device
// index (counts, offsets) and every key point's face are checked on the host before anything is enqueued (cms_sim3_opt_job_check.h).
#include <cstring>
#include <string>
#include <vector>
#include "cms_sim3_opt_job_check.h"

struct cms_sim3_opt : CmsRansacHandle {
  int max_corr = 0;
};

extern "C" int cms_sim3_opt_create(cms_sim3_opt** out, int device, int max_jobs, int max_corr_total) {
  if (!out || max_jobs < 1 || max_corr_total < 1) return cms_fail(CMS_ERR_ARG, "cms_sim3_opt_create: bad argument");
  const int rcd = cms_check_device(device, "cms_sim3_opt_create: no HIP device (OptimizeSim3's device path has no CPU fallback)");
  if (rcd) return rcd;
  cms_sim3_opt* p = new cms_sim3_opt();
  p->max_corr = max_corr_total;
  const int rc = p->open(device, max_jobs, true, "cms_sim3_opt_create");
  if (rc) { cms_ransac_free(p); return rc; }
  *out = p;
  return CMS_OK;
}
extern "C" void cms_sim3_opt_destroy(cms_sim3_opt* p) { cms_ransac_free(p); }

extern "C" int cms_sim3_optimize(cms_sim3_opt* p, cms_ctx* c, int njobs, cms_sim3_opt_job* jobs) {
  int rc = cms_ransac_check_entry(p, c, njobs, jobs, "cms_sim3_optimize");
  if (rc || njobs == 0) return rc;
  std::vector<CmsS3oJobDev> jd((size_t)njobs);
  long long corr = 0;
  for (int j = 0; j < njobs; ++j) {
    const cms_sim3_opt_job& q = jobs[j];
    const char* why = cms_sim3_opt_check_job(c->g.F, q);
    if (why) return cms_fail(CMS_ERR_ARG, (std::string("cms_sim3_optimize: ") + why).c_str());
    CmsS3oJobDev& d = jd[(size_t)j];
    d.N = q.N; d.corr0 = (int)corr; d.fix_scale = q.fix_scale ? 1 : 0; d.jacobian = q.jacobian; d.th2 = q.th2; d.pad = 0;
    std::memcpy(d.R, q.R12, sizeof(d.R)); std::memcpy(d.t, q.t12, sizeof(d.t)); d.s = q.s12;
    corr += q.N;
    if (corr > p->max_corr) return cms_fail(CMS_ERR_ARG, "cms_sim3_optimize: more correspondences than the handle was created for");
  }
  const size_t C_ = (size_t)corr, J_ = (size_t)njobs;
  CmsBlock blk;
  const size_t o_jobs = blk.take(J_ * sizeof(CmsS3oJobDev)), o_x1 = blk.take(C_ * 12), o_x2 = blk.take(C_ * 12), o_k1 = blk.take(C_ * 8), o_k2 = blk.take(C_ * 8),
               o_i1 = blk.take(C_ * 4), o_i2 = blk.take(C_ * 4);
  const size_t in_bytes = blk.size;
  const size_t o_out = blk.take(J_ * sizeof(CmsS3oOutDev)), o_keep = blk.take(C_);
  const size_t out_begin = o_out, out_end = blk.size;
  const size_t o_err = blk.take(C_ * 32);
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  rc = p->blocks.reserve(s, blk.size, out_end);
  if (rc) return rc;
  uint8_t* h = p->blocks.h;
  uint8_t* d = p->blocks.d;
  std::memset(h, 0, in_bytes);
  std::memcpy(h + o_jobs, jd.data(), J_ * sizeof(CmsS3oJobDev));
  for (int j = 0; j < njobs; ++j) {
    const cms_sim3_opt_job& q = jobs[j];
    if (q.N == 0) continue;
    const size_t c0 = (size_t)jd[(size_t)j].corr0, n = (size_t)q.N;
    std::memcpy(h + o_x1 + 12 * c0, q.x3dc1, 12 * n); std::memcpy(h + o_x2 + 12 * c0, q.x3dc2, 12 * n);
    std::memcpy(h + o_k1 + 8 * c0, q.kp1, 8 * n); std::memcpy(h + o_k2 + 8 * c0, q.kp2, 8 * n);
    std::memcpy(h + o_i1 + 4 * c0, q.inv_sigma2_1, 4 * n); std::memcpy(h + o_i2 + 4 * c0, q.inv_sigma2_2, 4 * n);
  }
  rc = p->blocks.up(s, in_bytes, "cms_sim3_optimize");
  if (rc) return rc;
  CmsS3oArgs a = {};
  a.F = c->g.F; a.njobs = njobs; a.jobs = (const CmsS3oJobDev*)(d + o_jobs);
  a.x1 = (const float*)(d + o_x1); a.x2 = (const float*)(d + o_x2); a.kp1 = (const float*)(d + o_k1); a.kp2 = (const float*)(d + o_k2);
  a.is1 = (const float*)(d + o_i1); a.is2 = (const float*)(d + o_i2);
  a.err = (double*)(d + o_err); a.keep = d + o_keep; a.out = (CmsS3oOutDev*)(d + o_out);
  hipLaunchKernelGGL(k_sim3_optimize, dim3(njobs), dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  rc = p->blocks.back_and_wait(s, out_begin, out_end, "cms_sim3_optimize");
  if (rc) return rc;
  for (int j = 0; j < njobs; ++j) {
    cms_sim3_opt_job& q = jobs[j];
    const CmsS3oOutDev& o = reinterpret_cast<const CmsS3oOutDev*>(h + o_out)[j];
    q.n_inliers = o.n_inliers; q.n_correspondences = o.n_correspondences; q.n_bad = o.n_bad; q.iterations[0] = o.its[0]; q.iterations[1] = o.its[1];
    std::memcpy(q.q12, o.q, sizeof(q.q12)); std::memcpy(q.t12_out, o.t, sizeof(q.t12_out)); q.s12_out = o.s;
    if (q.N > 0) std::memcpy(q.keep, h + o_keep + (size_t)jd[(size_t)j].corr0, (size_t)q.N);
  }
  return CMS_OK;
}
