// sim3_search_host.cpp -- the host build of csrc/cms_sim3_search_core.h and of the job check of cms_kfstore_search_by_sim3: what the CPU tests
// (tests/test_sim3_search_cpu.py) compare with the numpy restatement tests/npref_sim3_search.py.  No GPU is touched here.
#include <cstdio>
#include <cstring>
#include "cubemapslam_hip.h"
#include "../csrc/cms_sim3_search_core.h"
#include "../csrc/cms_sim3_search_job_check.h"

// sR12 (9) | t12 (3) | sR21 (9) | t21 (3) of one similarity
extern "C" void hm_sim3s_compose(float s12, const float* R12, const float* t12, float* out24) {
  CmsSim3sMotion m;
  cms_sim3s_compose(s12, R12, t12, &m);
  std::memcpy(out24, &m, sizeof(m));
}
extern "C" int hm_sim3s_motion_size() { return (int)sizeof(CmsSim3sMotion); }

// One direction for n map points of one key frame: pose12 = Rw | tw of the points' own key frame, sR | t the similarity into the other camera.
// why[i] is CMS_SIM3S_KEEP / _BEHIND / _IMAGE / _DIST.
extern "C" void hm_sim3s_project(int F, const float* pose12, const float* sR, const float* t, int second_as_depth, int bounds_scaled, int n, const float* pos,
                                 const float* min_dist, const float* max_dist, float* u, float* v, float* dist3D, float* raw_max, int* why) {
  for (int i = 0; i < n; ++i)
    why[i] = cms_sim3s_project(F, pose12, pose12 + 9, sR, t, pos + 3 * (size_t)i, second_as_depth, bounds_scaled, min_dist[i], max_dist[i], u + i, v + i, dist3D + i, raw_max + i);
}

// The checks of cms_kfstore_search_by_sim3 over a store described by plain arrays: used[maxkf], slot_n[maxkf] (the slots' stored key-point counts).
// Returns CMS_OK or CMS_ERR_ARG with the reason in `reason` (cap bytes).
extern "C" int hm_sim3s_job_check(int njobs, const cms_sim3_search_job* jobs, int maxkf, const uint8_t* used, const int* slot_n, int n_mp, float th, int nlevels,
                                  int same_device, char* reason, int cap) {
  const char* why = cms_sim3s_check_call(th, nlevels, same_device, n_mp);
  int cursor = 0;
  long long entries = 0;
  for (int j = 0; j < njobs && !why; ++j) why = cms_sim3s_check_job(jobs[j], maxkf, used, [&](int slot) { return slot_n[slot]; }, n_mp, &cursor, &entries);
  if (reason && cap > 0) std::snprintf(reason, (size_t)cap, "%s", why ? why : "");
  return why ? CMS_ERR_ARG : CMS_OK;
}
