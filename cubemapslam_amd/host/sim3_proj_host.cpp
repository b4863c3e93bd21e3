// sim3_proj_host.cpp -- the host build of csrc/cms_sim3_proj_core.h and of the job check of cms_kfstore_search_by_projection_sim3 /
// cms_kfstore_fuse_search_sim3: what the CPU tests (tests/test_sim3_projection_cpu.py) compare with the numpy restatement
// tests/npref_sim3_projection.py.  No GPU is touched here.
#include <cstdio>
#include <cstring>
#include "cubemapslam_hip.h"
#include "../csrc/cms_sim3_proj_core.h"
#include "../csrc/cms_sim3_proj_job_check.h"

// Rcw (9) | tcw (3) | Ow (3) | scw of one Scw (rows 0..2 of [sR | t], row major)
extern "C" void hm_sim3p_decompose(const float* Scw, float* out16) {
  CmsSim3pPose p;
  cms_sim3p_decompose(Scw, &p);
  std::memcpy(out16, &p, sizeof(p));
}
extern "C" int hm_sim3p_pose_size() { return (int)sizeof(CmsSim3pPose); }
extern "C" int hm_sim3p_job_size() { return (int)sizeof(cms_sim3_proj_job); }

// The chain over n points under one Scw.  sf: nlevels scale factors; log_scale: logf(sf[1]).  why[i] is CMS_SIM3P_KEEP / _BEHIND / _IMAGE / _DIST / _ANGLE.
extern "C" void hm_sim3p_project(int F, const float* Scw, int bounds_scaled, float th, float log_scale, int nlevels, const float* sf, int n, const float* pos,
                                 const float* normal, const float* min_dist, const float* max_dist, float* u, float* v, float* dist, int* level, float* radius, int* why) {
  CmsSim3pPose p;
  cms_sim3p_decompose(Scw, &p);
  for (int i = 0; i < n; ++i)
    why[i] = cms_sim3p_project(F, &p, pos + 3 * (size_t)i, normal + 3 * (size_t)i, bounds_scaled, min_dist[i], max_dist[i], th, log_scale, nlevels, sf, u + i, v + i, dist + i,
                               level + i, radius + i);
}

// The checks of the two entries over a store described by plain arrays: used[maxkf], slot_n[maxkf] (the slots' stored key-point counts).
// Returns CMS_OK or CMS_ERR_ARG with the reason in `reason` (cap bytes).
extern "C" int hm_sim3p_job_check(int njobs, const cms_sim3_proj_job* jobs, int maxkf, const uint8_t* used, const int* slot_n, int nsets, const int* set_off, float th,
                                  int nlevels, int same_device, char* reason, int cap) {
  const char* why = cms_sim3p_check_call(th, nlevels, same_device, nsets, set_off);
  long long entries = 0;
  for (int j = 0; j < njobs && !why; ++j) why = cms_sim3p_check_job(jobs[j], maxkf, used, [&](int slot) { return slot_n[slot]; }, nsets, set_off, &entries);
  if (reason && cap > 0) std::snprintf(reason, (size_t)cap, "%s", why ? why : "");
  return why ? CMS_ERR_ARG : CMS_OK;
}
