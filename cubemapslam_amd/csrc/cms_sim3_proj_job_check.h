// cms_sim3_proj_job_check.h -- what cms_kfstore_search_by_projection_sim3 and cms_kfstore_fuse_search_sim3 check before anything is enqueued or
// written.  Host code, shared by the C-ABI entries (cms_api_sim3_proj.hip) and the host library (host/sim3_proj_host.cpp: hm_sim3p_job_check), so
// both refuse the same records with the same words.  Needs cms_sim3_proj_job (include/cubemapslam_hip.h) before it.  Everything that becomes a
// device index passes through here: slots, set indices, the set offsets that size the entries.  A function returns NULL or the reason.
#ifndef CMS_SIM3_PROJ_JOB_CHECK_H
#define CMS_SIM3_PROJ_JOB_CHECK_H
#include <math.h>
#include <stdint.h>

#define CMS_SIM3P_MAX_ENTRIES (0x7FFFFFFF / 80)      /* entries of one call: 64 candidates each plus slack stay inside an int */
#define CMS_SIM3P_KPMAX 4096                         /* key points of one key frame the greedy kernel's claim tables (LDS) hold */

// the call's scalars and sets; same_device: the context and the store live on one device
static inline const char* cms_sim3p_check_call(float th, int nlevels, int same_device, int nsets, const int* set_off) {
  if (!same_device) return "the context and the store must share the device";
  if (!(th >= 0.0f) || !isfinite(th)) return "th must be finite and >= 0";
  if (nlevels > 16) return "more than 16 pyramid levels";
  if (nsets < 0 || (nsets > 0 && !set_off)) return "bad sets";
  if (nsets > 0 && set_off[0] != 0) return "set offsets must start at 0";
  for (int s = 0; s < nsets; ++s)
    if (set_off[s + 1] < set_off[s]) return "set offsets must ascend";
  return nullptr;
}

// One job.  used[slot] != 0: the slot is filled; slot_n(slot): its stored key-point count.  *entries: the call's entries so far.
template <class SlotN>
static inline const char* cms_sim3p_check_job(const cms_sim3_proj_job& q, int maxkf, const uint8_t* used, SlotN&& slot_n, int nsets, const int* set_off, long long* entries) {
  if (q.slot < 0 || q.slot >= maxkf) return "slot out of range";
  if (!used[q.slot]) return "empty slot";
  if (q.n < 0 || q.n != slot_n(q.slot)) return "n is not the slot's stored key-point count";
  if (q.set < 0 || q.set >= nsets) return "set out of range";
  for (int k = 0; k < 12; ++k)
    if (!isfinite(q.Scw[k])) return "Scw must be finite";
  double d = 0.0;
  for (int k = 0; k < 3; ++k) d = d + (double)q.Scw[k] * (double)q.Scw[k];
  const float scw = (float)sqrt(d);
  if (!isfinite(scw) || scw == 0.0f) return "scw must be finite and nonzero";
  *entries += (long long)set_off[q.set + 1] - set_off[q.set];
  if (*entries > CMS_SIM3P_MAX_ENTRIES) return "too many entries for one call";
  return nullptr;
}

#endif
