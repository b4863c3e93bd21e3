// cms_sim3_search_job_check.h -- what cms_kfstore_search_by_sim3 checks before anything is enqueued.  Host code, shared by the C-ABI entry
// (cms_api_sim3_search.hip) and the host library (host/sim3_search_host.cpp: hm_sim3s_job_check), so both refuse the same records with the same
// words.  Needs cms_sim3_search_job (include/cubemapslam_hip.h) before it.  Everything that becomes a device index passes through here: slots, the
// key-point counts that size the entries, and the offsets into the map-point arrays.  A function returns NULL or the reason.
#ifndef CMS_SIM3_SEARCH_JOB_CHECK_H
#define CMS_SIM3_SEARCH_JOB_CHECK_H
#include <math.h>
#include <stdint.h>

#define CMS_SIM3S_MAX_ENTRIES (0x7FFFFFFF / 80)      /* entries of one call: 64 candidates each plus slack stay inside an int */

// the call's scalars; same_device: the context and the store live on one device
static inline const char* cms_sim3s_check_call(float th, int nlevels, int same_device, int n_mp) {
  if (!same_device) return "the context and the store must share the device";
  if (!(th >= 0.0f) || !isfinite(th)) return "th must be finite and >= 0";
  if (nlevels > 16) return "more than 16 pyramid levels";
  if (n_mp < 0) return "n_mp is negative";
  return nullptr;
}

// One job.  used[slot] != 0: the slot is filled; slot_n(slot): its stored key-point count.  *cursor: where the previous job's map-point records end
// (0 before the first job), moved behind this job's; *entries: the call's entries so far.
template <class SlotN>
static inline const char* cms_sim3s_check_job(const cms_sim3_search_job& q, int maxkf, const uint8_t* used, SlotN&& slot_n, int n_mp, int* cursor, long long* entries) {
  const int slots[2] = {q.slot1, q.slot2}, counts[2] = {q.n1, q.n2};
  for (int k = 0; k < 2; ++k) {
    if (slots[k] < 0 || slots[k] >= maxkf) return "slot out of range";
    if (!used[slots[k]]) return "empty slot";
    if (counts[k] < 0 || counts[k] != slot_n(slots[k])) return "n1 / n2 is not the slot's stored key-point count";
  }
  if (!isfinite(q.s12) || q.s12 == 0.0f) return "s12 must be finite and nonzero";
  // key frame 1's records, then key frame 2's, job after job: [off1, off1 + n1) <= [off2, off2 + n2) <= n_mp, nothing before *cursor
  if (q.off1 < *cursor || q.off1 > n_mp || q.n1 > n_mp - q.off1) return "off1 does not ascend or reaches beyond n_mp";
  if (q.off2 < q.off1 + q.n1 || q.off2 > n_mp || q.n2 > n_mp - q.off2) return "off2 does not ascend or reaches beyond n_mp";
  *cursor = q.off2 + q.n2;
  *entries += (long long)q.n1 + q.n2;
  if (*entries > CMS_SIM3S_MAX_ENTRIES) return "too many key points for one call";
  return nullptr;
}

#endif
