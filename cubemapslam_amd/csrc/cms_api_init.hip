// cms_api_init.hip -- host side of the Initializer (src/Initializer.cpp): the cms_init handle, cms_init_two_view and cms_init_two_view_frames
// (k_init_gather in front); included by cms_lib.hip behind cms_api_frames.hip (cms_ctx, cms_fail, HIPCHK, CmsBlock) and cms_init_kernels.hip.  All
// jobs of a call are ONE launch sequence on the context's stream: one pinned block up (the handle's CmsStage), k_init_hypotheses, k_init_check, k_init_select, one pinned
// block back; ReconstructE's decision (cms_init_core.h, host only) is then taken per job.  Everything that becomes a device index (draws, match
// indices, counts, offsets) is checked on the host before anything is enqueued (cms_init_job_check.h).  The handle base, the head of an entry and the
// staging of the draws are cms_api_ransac.h, shared with the PnP and Sim3 entries.
#include <cstring>
#include <vector>
#include "cms_init_job_check.h"

struct cms_init : CmsRansacHandle {      // no stream of its own: the entries run on the context's
  int max_matches = 0, max_keys1 = 0, max_hyp = 0;
};

extern "C" int cms_init_create(int device, int max_jobs, int max_matches_total, int max_keys1_total, int max_hyp_total, cms_init** out) {
  if (!out || max_jobs < 1 || max_matches_total < 1 || max_keys1_total < 1 || max_hyp_total < 1) return cms_fail(CMS_ERR_ARG, "cms_init_create: bad argument");
  const int rcd = cms_check_device(device, "cms_init_create: no HIP device (the initializer's device path has no CPU fallback)");
  if (rcd) return rcd;
  cms_init* p = new cms_init();
  p->max_matches = max_matches_total; p->max_keys1 = max_keys1_total; p->max_hyp = max_hyp_total;
  (void)p->open(device, max_jobs, false, "cms_init_create");
  *out = p;
  return CMS_OK;
}
extern "C" void cms_init_destroy(cms_init* p) { cms_ransac_free(p); }

// frames: cms_init_two_view_frames -- frame 2 is gathered on the device from the context's resident rows
static int cms_init_run(cms_init* p, cms_ctx* c, int njobs, cms_init_job* jobs, bool frames) {
  int rc = cms_ransac_check_entry(p, c, njobs, jobs, "cms_init_two_view");
  if (rc || njobs == 0) return rc;
  std::vector<CmsInitJobDev> jd((size_t)njobs);
  long long nm = 0, hyp = 0, words = 0, nk = 0;
  for (int j = 0; j < njobs; ++j) {
    int N = 0;
    rc = cms_init_check_job(jobs[j], &N, frames);
    if (rc) return cms_fail(rc, "cms_init_two_view: bad job (null array, fewer than 8 matches, a match index outside [-1, n2), iterations < 1, fewer than 8*iterations draws, or a draw outside [0, N-1-k])");
    const cms_init_job& q = jobs[j];
    if (frames && (q.b >= c->max_batch || q.n2 > c->g.kp_cap)) return cms_fail(CMS_ERR_ARG, "cms_init_two_view_frames: frame row or key-point count beyond the context's");
    CmsInitJobDev& d = jd[(size_t)j];
    d.N = N; d.H = q.iterations; d.n1 = q.n1; d.m0 = (int)nm; d.hyp0 = (int)hyp; d.key0 = (int)nk; d.words = (N + 63) / 64; d.word0 = words;
    d.sigma = q.sigma; d.th2 = cms_init_th2(q.sigma);
    nm += N; hyp += q.iterations; words += (long long)q.iterations * d.words; nk += q.n1;
    if (nm > p->max_matches) return cms_fail(CMS_ERR_ARG, "cms_init_two_view: more matches than the handle was created for");
    if (nk > p->max_keys1) return cms_fail(CMS_ERR_ARG, "cms_init_two_view: more key points of the reference frames than the handle was created for");
    if (hyp > p->max_hyp) return cms_fail(CMS_ERR_ARG, "cms_init_two_view: more hypotheses than the handle was created for");
  }
  const size_t M = (size_t)nm, Hn = (size_t)hyp, J_ = (size_t)njobs, K1 = (size_t)nk;
  CmsBlock blk;
  const size_t o_jobs = blk.take(J_ * sizeof(CmsInitJobDev)), o_hjob = blk.take(Hn * 4), o_draws = blk.take(Hn * 32), o_first = blk.take(M * 4), o_ray1 = blk.take(M * 12),
               o_kp1 = blk.take(M * 8), o_ray2 = blk.take(M * 12), o_kp2 = blk.take(M * 8), o_second = blk.take(M * 4), o_mjob = blk.take(M * 4), o_jrow = blk.take(J_ * 4);
  const size_t in_bytes = blk.size;
  const size_t o_out = blk.take(J_ * sizeof(CmsInitOutDev)), o_p3d = blk.take(K1 * 48), o_good = blk.take(K1 * 4);
  const size_t out_begin = o_out, out_end = blk.size;
  const size_t o_E = blk.take(Hn * 36), o_score = blk.take(Hn * 4), o_hmask = blk.take((size_t)words * 8), o_keys = blk.take(M * 4);
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = c->stream;
  rc = p->blocks.reserve(s, blk.size, out_end);
  if (rc) return rc;
  uint8_t* h = p->blocks.h;
  uint8_t* d = p->blocks.d;
  std::memset(h, 0, in_bytes);
  std::memcpy(h + o_jobs, jd.data(), J_ * sizeof(CmsInitJobDev));
  for (int j = 0; j < njobs; ++j) {
    const cms_init_job& q = jobs[j];
    const CmsInitJobDev& g = jd[(size_t)j];
    cms_ransac_stage_draws<8>(reinterpret_cast<int*>(h + o_hjob) + g.hyp0, reinterpret_cast<int*>(h + o_draws) + 8 * (size_t)g.hyp0, j, g.H, q.draws);
    reinterpret_cast<int*>(h + o_jrow)[j] = frames ? q.b : 0;
    int* first = reinterpret_cast<int*>(h + o_first) + g.m0;
    int* second = reinterpret_cast<int*>(h + o_second) + g.m0;
    int* mjob = reinterpret_cast<int*>(h + o_mjob) + g.m0;
    float* ray1 = reinterpret_cast<float*>(h + o_ray1) + 3 * (size_t)g.m0;
    float* kp1 = reinterpret_cast<float*>(h + o_kp1) + 2 * (size_t)g.m0;
    float* ray2 = reinterpret_cast<float*>(h + o_ray2) + 3 * (size_t)g.m0;
    float* kp2 = reinterpret_cast<float*>(h + o_kp2) + 2 * (size_t)g.m0;
    size_t k = 0;
    for (int i = 0; i < q.n1; ++i) {      // mvMatches12 (:61-73)
      const int i2 = q.matches12[i];
      if (i2 < 0) continue;
      first[k] = i; second[k] = i2; mjob[k] = j;
      std::memcpy(ray1 + 3 * k, q.rays1 + 3 * (size_t)i, 12); std::memcpy(kp1 + 2 * k, q.keys1 + 2 * (size_t)i, 8);
      if (!frames) { std::memcpy(ray2 + 3 * k, q.rays2 + 3 * (size_t)i2, 12); std::memcpy(kp2 + 2 * k, q.keys2 + 2 * (size_t)i2, 8); }
      ++k;
    }
  }
  rc = p->blocks.up(s, in_bytes, "cms_init_two_view");
  if (rc) return rc;
  if (frames) {
    CmsInitGatherArgs ga = {};
    ga.nmatch = (int)nm; ga.kp_cap = c->g.kp_cap;
    ga.m_job = (const int*)(d + o_mjob); ga.job_row = (const int*)(d + o_jrow); ga.m_second = (const int*)(d + o_second);
    ga.kps = (const CmsKeyPoint*)c->d_kps; ga.rays = c->d_rays;
    ga.m_ray2 = (float*)(d + o_ray2); ga.m_kp2 = (float*)(d + o_kp2);
    hipLaunchKernelGGL(k_init_gather, dim3(((int)nm + 255) / 256), dim3(256), 0, s, ga);
    HIPCHK(hipGetLastError());
  }
  CmsInitRunArgs a = {};
  a.F = c->g.F; a.njobs = njobs; a.nhyp = (int)hyp; a.cos_fov = cms_cos_fov(c);
  a.jobs = (const CmsInitJobDev*)(d + o_jobs); a.hyp_job = (const int*)(d + o_hjob); a.draws = (const int*)(d + o_draws);
  a.m_first = (const int*)(d + o_first); a.m_ray1 = (const float*)(d + o_ray1); a.m_kp1 = (const float*)(d + o_kp1);
  a.m_ray2 = (const float*)(d + o_ray2); a.m_kp2 = (const float*)(d + o_kp2);
  a.hyp_E = (float*)(d + o_E); a.hyp_score = (float*)(d + o_score); a.hyp_mask = (unsigned long long*)(d + o_hmask); a.cos_keys = (unsigned*)(d + o_keys);
  a.cand_p3d = (float*)(d + o_p3d); a.cand_good = d + o_good; a.out = (CmsInitOutDev*)(d + o_out);
  hipLaunchKernelGGL(k_init_hypotheses, dim3(((int)hyp + CMS_INIT_HYP_LANES - 1) / CMS_INIT_HYP_LANES), dim3(CMS_INIT_HYP_LANES), 0, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_init_check, dim3((int)hyp), dim3(64), 0, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_init_select, dim3(njobs), dim3(CMS_INIT_SELECT_THREADS), 0, s, a);
  HIPCHK(hipGetLastError());
  rc = p->blocks.back_and_wait(s, out_begin, out_end, "cms_init_two_view");
  if (rc) return rc;
  for (int j = 0; j < njobs; ++j) {
    const CmsInitJobDev& g = jd[(size_t)j];
    const CmsInitOutDev& o = reinterpret_cast<const CmsInitOutDev*>(h + o_out)[j];
    cms_init_finish_job(jobs[j], o.best, o.score, o.n_inliers, o.nGood, o.cosines, o.R1, o.R2, o.t, reinterpret_cast<const float*>(h + o_p3d) + 12 * (size_t)g.key0,
                        h + o_good + 4 * (size_t)g.key0);
  }
  return CMS_OK;
}

extern "C" int cms_init_two_view(cms_init* p, cms_ctx* c, int njobs, cms_init_job* jobs) { return cms_init_run(p, c, njobs, jobs, false); }
extern "C" int cms_init_two_view_frames(cms_init* p, cms_ctx* c, int njobs, cms_init_job* jobs) { return cms_init_run(p, c, njobs, jobs, true); }
