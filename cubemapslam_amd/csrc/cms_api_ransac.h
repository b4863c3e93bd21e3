// cms_api_ransac.h -- what the host sides of the three RANSAC solvers share (cms_api_pnp.hip, cms_api_init.hip, cms_api_sim3.hip): the handle
// base, the check at the head of an entry and the staging of a job's draws.  Included by cms_lib.hip behind cms_api_frames.hip (cms_ctx,
// cms_fail, HIPCHK, CmsStage).  Layouts, gathers, launches and the unpacking of results are each solver's own.
#pragma once
#include <cstring>
#include <string>

// cms_pnp, cms_sim3 and cms_init derive from this and add their capacities
struct CmsRansacHandle {
  int device = 0, max_jobs = 0;
  hipStream_t stream = nullptr;      // the handle's own stream, for the entries that do not run on the context's
  CmsStage blocks;                   // one device block and one pinned block, grown on demand

  // behind the entry's argument and device checks; a failure leaves a handle that cms_ransac_free takes
  int open(int device_, int max_jobs_, bool own_stream, const char* who) {
    device = device_; max_jobs = max_jobs_;
    if (!own_stream) return CMS_OK;
    HIPCHK(hipSetDevice(device));
    if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return cms_fail(CMS_ERR_HIP, (std::string(who) + ": hipStreamCreate").c_str());
    return CMS_OK;
  }
};
template <class Handle>
static void cms_ransac_free(Handle* p) {
  if (!p) return;
  hipSetDevice(p->device);
  p->blocks.release();
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

// The head of an entry.  The caller returns on a refusal and on njobs == 0 alike: `if (rc || njobs == 0) return rc;`
static int cms_ransac_check_entry(const CmsRansacHandle* p, const cms_ctx* c, int njobs, const void* jobs, const char* who) {
  const char* why = nullptr;
  if (!p || !c || njobs < 0 || (njobs > 0 && !jobs)) why = ": bad argument";
  else if (njobs == 0) return CMS_OK;
  else if (c->device != p->device) why = ": the context and the handle must share the device";
  else if (njobs > p->max_jobs) why = ": more jobs than the handle was created for";
  return why ? cms_fail(CMS_ERR_ARG, (std::string(who) + why).c_str()) : CMS_OK;
}

// Job j's part of the call's hypothesis arrays: hyp_job and draws_out point at the job's first hypothesis (hyp0, K * hyp0)
template <int K>
static void cms_ransac_stage_draws(int* hyp_job, int* draws_out, int j, int H, const int* draws) {
  for (int k = 0; k < H; ++k) hyp_job[k] = j;
  if (H > 0) std::memcpy(draws_out, draws, sizeof(int) * K * (size_t)H);
}
