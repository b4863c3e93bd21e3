// cms_api_sim3_search.hip -- host side of ORBMatcher::SearchBySim3 on resident key frames (cms_kfstore_search_by_sim3); included by cms_lib.hip
// behind cms_api_tri.hip (cms_kfstore, kfstore_wait_puts), cms_api_area.hip (the window query's launcher) and cms_sim3_search_kernels.hip.  All jobs
// of a call are ONE launch sequence on src's stream with src's staging block, like kfstore_fuse_core on the store's: k_sim3s_project, the window
// query against the store's grids, k_sim3s_scan, k_sim3s_agree; the candidate total is read together with the results (one synchronisation) and a
// call whose lists did not fit is repeated by cms_retry_capacity.  Everything that becomes a device index is checked before anything is enqueued
// (cms_sim3_search_job_check.h).
#include <cstring>
#include <string>
#include <vector>
#include "cms_sim3_search_job_check.h"

extern "C" int cms_kfstore_search_by_sim3(cms_kfstore* st, cms_ctx* src, int njobs, const cms_sim3_search_job* jobs, int n_mp, const uint8_t* skip, const float* pos,
                                          const float* min_dist, const float* max_dist, const uint8_t* mp_desc, float th, int z_as_written, int* idx2, int* n_found) {
  const char* who = "cms_kfstore_search_by_sim3";
  auto refuse = [&](const char* why) { return cms_fail(CMS_ERR_ARG, (std::string(who) + ": " + why).c_str()); };
  if (!st || !src || njobs < 0 || (njobs > 0 && (!jobs || !n_found))) return refuse("bad argument");
  if (njobs == 0) return CMS_OK;
  const cms_ctx* g = st->c;                                        // the geometry the slots' grids were built with
  const char* why = cms_sim3s_check_call(th, g->g.nlevels, src->device == g->device, n_mp);
  if (why) return refuse(why);
  int cursor = 0;
  long long entries = 0;
  std::vector<CmsSim3sJobDev> jd((size_t)njobs);
  std::vector<int> ent_off((size_t)njobs + 1, 0), n1_off((size_t)njobs + 1, 0);
  for (int j = 0; j < njobs; ++j) {
    const cms_sim3_search_job& q = jobs[j];
    why = cms_sim3s_check_job(q, st->maxkf, st->used.data(), [&](int slot) { return st->h_kf[(size_t)slot].n; }, n_mp, &cursor, &entries);
    if (why) return refuse(why);
    CmsSim3sJobDev& d = jd[(size_t)j];
    d.slot1 = q.slot1; d.slot2 = q.slot2; d.n1 = q.n1; d.n2 = q.n2; d.off1 = q.off1; d.off2 = q.off2;
    const CmsTriKF& k1 = st->h_kf[(size_t)q.slot1];
    const CmsTriKF& k2 = st->h_kf[(size_t)q.slot2];
    std::memcpy(d.R1w, k1.Rcw, 36); std::memcpy(d.t1w, k1.tcw, 12); std::memcpy(d.R2w, k2.Rcw, 36); std::memcpy(d.t2w, k2.tcw, 12);
    cms_sim3s_compose(q.s12, q.R12, q.t12, &d.m);
    ent_off[(size_t)j + 1] = ent_off[(size_t)j] + q.n1 + q.n2;
    n1_off[(size_t)j + 1] = n1_off[(size_t)j] + q.n1;
  }
  const int E = ent_off[(size_t)njobs], N1 = n1_off[(size_t)njobs];
  if (E > 0 && (!skip || !pos || !min_dist || !max_dist || !mp_desc)) return refuse("bad map-point arrays");
  if (N1 > 0 && !idx2) return refuse("bad argument");
  for (int j = 0; j < njobs; ++j) n_found[j] = 0;                   // (nothing of the caller's is written before the last check has passed)
  for (int i = 0; i < N1; ++i) idx2[i] = -1;
  if (E == 0 || N1 == 0 || N1 == E) return CMS_OK;                  // a side without key points in every job: no match anywhere
  HIPCHK(hipSetDevice(src->device));
  hipStream_t s = src->stream;
  int rc = kfstore_wait_puts(st, s, 2 * njobs, [&](int j) { return (j & 1) ? jobs[j >> 1].slot2 : jobs[j >> 1].slot1; });
  if (rc) return rc;
  const size_t e4 = (size_t)E * 4, j4 = (size_t)njobs * 4, m4 = (size_t)n_mp * 4;
  CmsBlock blk;
  CmsWindowCols w;      // (slot: the OTHER key frame's; rec: the entry's map-point record)
  const size_t o_job = blk.take(jd.size() * sizeof(CmsSim3sJobDev)), o_eoff = blk.take(j4, 4), o_noff = blk.take(j4, 4), o_skip = blk.take((size_t)n_mp), o_pos = blk.take(3 * m4),
               o_min = blk.take(m4), o_max = blk.take(m4), o_desc = blk.take((size_t)n_mp * 32), o_match = blk.take(e4), o_idx2 = blk.take((size_t)N1 * 4),
               o_tot = blk.take(4 + j4);      // the total, then n_found
  w.take(blk, (size_t)E);
  const size_t o_idx = blk.size;
  const bool direct = cms_is_pinned(idx2);      // k_sim3s_agree stores there itself
  std::vector<int> back((size_t)njobs + 1);
  rc = cms_retry_capacity(64 * E + 1024, who, [&](int cap, int& tot) -> int {
    int rr = src->stage.reserve(s, o_idx + cms_align((size_t)cap * 4), 0);
    if (rr) return rr;
    uint8_t* p = src->stage.d;
    w.at(p, o_idx);
    HIPCHK(hipMemcpyAsync(p + o_job, jd.data(), jd.size() * sizeof(CmsSim3sJobDev), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_eoff, ent_off.data(), j4 + 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_noff, n1_off.data(), j4 + 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_skip, skip, (size_t)n_mp, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_pos, pos, 3 * m4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_min, min_dist, m4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_max, max_dist, m4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_desc, mp_desc, (size_t)n_mp * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(p + o_tot, 0, 4 + j4, s));
    CmsSim3sArgs a = {};
    a.n_ent = E; a.njobs = njobs; a.job = (const CmsSim3sJobDev*)(p + o_job); a.ent_off = (const int*)(p + o_eoff);
    a.skip = p + o_skip; a.pos = (const float*)(p + o_pos); a.min_dist = (const float*)(p + o_min); a.max_dist = (const float*)(p + o_max);
    a.th = th; a.log_scale = cms_log_scale(g); a.nlevels = g->g.nlevels; a.F = g->g.F;
    a.bounds_scaled = src->dist_bounds_scaled; a.z_as_written = z_as_written ? 1 : 0;
    cms_level_table(a.sf, g, g->scale, 0.0f);
    a.qx = w.qx; a.qy = w.qy; a.qr = w.qr; a.qmin = w.qmin; a.qmax = w.qmax; a.level = w.level; a.qslot = w.slot; a.rec = w.rec;
    hipLaunchKernelGGL(k_sim3s_project, dim3((E + 255) / 256), dim3(256), 0, s, a);
    rr = kfstore_window_query(st, src, s, w, E, cap, p + o_tot);
    if (rr) return rr;
    // the scan and the agreement are enqueued right behind the windows: the total is looked at together with the results (the list kernel never
    // writes beyond `cap`, the scan never reads beyond it, and a call whose lists did not fit is simply repeated with room for them)
    const CmsWindowScanArgs sa = cms_window_scan_args(g, E, w, cap, w.rec, p + o_desc, st->d_kp, st->d_desc, w.slot, st->maxf, (int*)(p + o_match), nullptr);
    hipLaunchKernelGGL(k_sim3s_scan, dim3(cms_window_scan_grid(E)), dim3(256), 0, s, sa);
    CmsSim3sAgreeArgs ga = {};
    ga.n1_total = N1; ga.njobs = njobs; ga.job = a.job; ga.ent_off = a.ent_off; ga.n1_off = (const int*)(p + o_noff); ga.match = sa.best_idx;
    ga.idx2 = direct ? idx2 : (int*)(p + o_idx2); ga.n_found = (int*)(p + o_tot) + 1;
    hipLaunchKernelGGL(k_sim3s_agree, dim3((N1 + 255) / 256), dim3(256), 0, s, ga);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(back.data(), p + o_tot, 4 + j4, hipMemcpyDeviceToHost, s));
    if (!direct) HIPCHK(hipMemcpyAsync(idx2, p + o_idx2, (size_t)N1 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    tot = back[0];
    return CMS_OK;
  });
  if (rc) return rc;
  std::memcpy(n_found, back.data() + 1, j4);
  return CMS_OK;
}
