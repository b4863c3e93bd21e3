// cms_api_sim3_proj.hip -- host side of ORBMatcher::SearchByProjection(KeyFrame*, Scw, ...) and of the search half of ORBMatcher::Fuse(KeyFrame*, Scw, ...)
// on resident key frames (cms_kfstore_search_by_projection_sim3, cms_kfstore_fuse_search_sim3); included by cms_lib.hip behind cms_api_tri.hip
// (cms_kfstore, kfstore_wait_puts, kfstore_window_query, cms_window_scan_args), cms_api_area.hip (CmsWindowCols) and cms_sim3_proj_kernels.hip.  Both entries are one body, sim3p_core: all jobs of a call are ONE launch sequence on src's stream with src's staging
// block, as cms_kfstore_search_by_sim3 runs -- k_sim3p_project, the window query against the store's grids, then k_sim3p_greedy or k_sim3p_scan; the
// candidate total is read together with the results (one synchronisation) and a call whose lists did not fit is repeated by cms_retry_capacity.
// Everything that becomes a device index is checked before anything is enqueued or written (cms_sim3_proj_job_check.h).
#include <cstring>
#include <string>
#include <vector>
#include "cms_sim3_proj_job_check.h"

static thread_local int g_sim3p_last_rounds = 0;      // most rounds a job of this thread's last SearchByProjection call needed

// greedy: SearchByProjection (out_a = match_kp, out_b = NULL, n_matches); else Fuse (out_a = best_idx, out_b = best_dist)
static int sim3p_core(const char* who, bool greedy, cms_kfstore* st, cms_ctx* src, int nsets, const int* set_off, const float* pos, const float* normal, const float* min_dist,
                      const float* max_dist, const uint8_t* mp_desc, int njobs, const cms_sim3_proj_job* jobs, const uint8_t* skip, const uint8_t* taken, float th, int* out_a,
                      int* out_b, int* n_matches) {
  auto refuse = [&](const char* why) { return cms_fail(CMS_ERR_ARG, (std::string(who) + ": " + why).c_str()); };
  if (!st || !src || njobs < 0 || (njobs > 0 && (!jobs || (greedy && !n_matches)))) return refuse("bad argument");
  if (njobs == 0) return CMS_OK;
  const cms_ctx* g = st->c;                                        // the geometry the slots' grids were built with
  const char* why = cms_sim3p_check_call(th, g->g.nlevels, src->device == g->device, nsets, set_off);
  if (why) return refuse(why);
  if (greedy && st->maxf > CMS_SIM3P_KPMAX) return refuse("the store's max_features exceeds the claim table (4096)");
  long long entries = 0;
  std::vector<CmsSim3pJobDev> jd((size_t)njobs);
  std::vector<int> ent_off((size_t)njobs + 1, 0);
  int T = 0;
  for (int j = 0; j < njobs; ++j) {
    const cms_sim3_proj_job& q = jobs[j];
    why = cms_sim3p_check_job(q, st->maxkf, st->used.data(), [&](int slot) { return st->h_kf[(size_t)slot].n; }, nsets, set_off, &entries);
    if (why) return refuse(why);
    CmsSim3pJobDev& d = jd[(size_t)j];
    d.slot = q.slot; d.n = q.n; d.set0 = set_off[q.set]; d.taken0 = T;
    cms_sim3p_decompose(q.Scw, &d.ps);
    ent_off[(size_t)j + 1] = (int)entries;
    T += q.n;
  }
  const int E = ent_off[(size_t)njobs], M = set_off[nsets];
  if (E > 0 && (!pos || !normal || !min_dist || !max_dist || !mp_desc || !out_a || (!greedy && !out_b))) return refuse("null array where entries exist");
  if (greedy && T > 0 && !taken) return refuse("null array where entries exist");
  if (greedy) for (int j = 0; j < njobs; ++j) n_matches[j] = 0;    // (nothing of the caller's is written before the last check has passed)
  for (int i = 0; i < E; ++i) { out_a[i] = -1; if (out_b) out_b[i] = 256; }
  if (E == 0 || T == 0) return CMS_OK;                             // no entries, or no key points in any job: no match anywhere
  HIPCHK(hipSetDevice(src->device));
  hipStream_t s = src->stream;
  int rc = kfstore_wait_puts(st, s, njobs, [&](int j) { return jobs[j].slot; });
  if (rc) return rc;
  const size_t e4 = (size_t)E * 4, j4 = (size_t)njobs * 4, m4 = (size_t)M * 4;
  CmsBlock blk;
  CmsWindowCols w;      // (slot: the job's; rec: the set's record an entry stands for)
  const size_t o_job = blk.take(jd.size() * sizeof(CmsSim3pJobDev)), o_eoff = blk.take(j4, 4), o_skip = blk.take((size_t)E), o_pos = blk.take(3 * m4), o_nrm = blk.take(3 * m4),
               o_min = blk.take(m4), o_max = blk.take(m4), o_desc = blk.take((size_t)M * 32), o_taken = blk.take((size_t)T), o_why = blk.take(e4), o_a = blk.take(e4),
               o_b = blk.take(e4), o_tot = blk.take(4 + 2 * j4);      // the total, n_matches, rounds
  w.take(blk, (size_t)E);
  const size_t o_idx = blk.size;
  // results in pinned (device-visible) host memory: the last kernel stores there itself
  const bool direct = cms_is_pinned(out_a) && (greedy || cms_is_pinned(out_b));
  std::vector<int> back(1 + 2 * (size_t)njobs);
  rc = cms_retry_capacity(64 * E + 1024, who, [&](int cap, int& tot) -> int {
    const size_t o_pd = o_idx + cms_align((size_t)cap * 4);
    int rr = src->stage.reserve(s, o_pd + cms_align((size_t)cap * 2), 0);
    if (rr) return rr;
    uint8_t* p = src->stage.d;
    w.at(p, o_idx);
    HIPCHK(hipMemcpyAsync(p + o_job, jd.data(), jd.size() * sizeof(CmsSim3pJobDev), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_eoff, ent_off.data(), j4 + 4, hipMemcpyHostToDevice, s));
    if (skip) HIPCHK(hipMemcpyAsync(p + o_skip, skip, (size_t)E, hipMemcpyHostToDevice, s));
    else HIPCHK(hipMemsetAsync(p + o_skip, 0, (size_t)E, s));
    HIPCHK(hipMemcpyAsync(p + o_pos, pos, 3 * m4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_nrm, normal, 3 * m4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_min, min_dist, m4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_max, max_dist, m4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(p + o_desc, mp_desc, (size_t)M * 32, hipMemcpyHostToDevice, s));
    if (greedy) HIPCHK(hipMemcpyAsync(p + o_taken, taken, (size_t)T, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(p + o_tot, 0, 4 + 2 * j4, s));
    CmsSim3pArgs a = {};
    a.n_ent = E; a.njobs = njobs; a.job = (const CmsSim3pJobDev*)(p + o_job); a.ent_off = (const int*)(p + o_eoff); a.skip = p + o_skip;
    a.pos = (const float*)(p + o_pos); a.normal = (const float*)(p + o_nrm); a.min_dist = (const float*)(p + o_min); a.max_dist = (const float*)(p + o_max);
    a.th = th; a.log_scale = cms_log_scale(g); a.nlevels = g->g.nlevels; a.F = g->g.F; a.bounds_scaled = src->dist_bounds_scaled;
    cms_level_table(a.sf, g, g->scale, 0.0f);
    a.qx = w.qx; a.qy = w.qy; a.qr = w.qr; a.qmin = w.qmin; a.qmax = w.qmax; a.level = w.level; a.qslot = w.slot; a.rec = w.rec; a.why = (int*)(p + o_why);
    hipLaunchKernelGGL(k_sim3p_project, dim3((E + 255) / 256), dim3(256), 0, s, a);
    rr = kfstore_window_query(st, src, s, w, E, cap, p + o_tot);
    if (rr) return rr;
    // the scan is enqueued right behind the windows: the total is looked at together with the results (the list kernel never writes beyond `cap`,
    // the scans never read beyond it, and a call whose lists did not fit is simply repeated with room for them)
    if (greedy) {
      CmsSim3pGreedyArgs ga = {};
      ga.job = a.job; ga.ent_off = a.ent_off; ga.level = a.level; ga.rec = a.rec; ga.mp_desc = (const uint4*)(p + o_desc); ga.cand_off = w.off;
      ga.cand_idx = w.idx; ga.cap = cap; ga.total = (const int*)(p + o_tot); ga.kp = st->d_kp; ga.t_desc = (const uint4*)st->d_desc; ga.maxf = st->maxf;
      ga.taken = p + o_taken; ga.pair_dist = (uint16_t*)(p + o_pd); ga.match = (int*)(p + o_a); ga.out = direct ? out_a : (int*)(p + o_a);
      ga.n_matches = (int*)(p + o_tot) + 1; ga.rounds = (int*)(p + o_tot) + 1 + njobs;
      hipLaunchKernelGGL(k_sim3p_greedy, dim3(njobs), dim3(1024), 0, s, ga);
    } else {
      const CmsWindowScanArgs sa = cms_window_scan_args(g, E, w, cap, w.rec, p + o_desc, st->d_kp, st->d_desc, w.slot, st->maxf, direct ? out_a : (int*)(p + o_a),
                                                        direct ? out_b : (int*)(p + o_b));
      hipLaunchKernelGGL(k_sim3p_scan, dim3(cms_window_scan_grid(E)), dim3(256), 0, s, sa);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(back.data(), p + o_tot, 4 + 2 * j4, hipMemcpyDeviceToHost, s));
    if (!direct) {
      HIPCHK(hipMemcpyAsync(out_a, p + o_a, e4, hipMemcpyDeviceToHost, s));
      if (!greedy) HIPCHK(hipMemcpyAsync(out_b, p + o_b, e4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    tot = back[0];
    return CMS_OK;
  });
  if (rc) return rc;
  if (greedy) {
    std::memcpy(n_matches, back.data() + 1, j4);
    int mx = 0;
    for (int j = 0; j < njobs; ++j) mx = back[1 + (size_t)njobs + j] > mx ? back[1 + (size_t)njobs + j] : mx;
    g_sim3p_last_rounds = mx;
  }
  return CMS_OK;
}

extern "C" int cms_kfstore_search_by_projection_sim3(cms_kfstore* st, cms_ctx* src, int nsets, const int* set_off, const float* pos, const float* normal, const float* min_dist,
                                                     const float* max_dist, const uint8_t* mp_desc, int njobs, const cms_sim3_proj_job* jobs, const uint8_t* skip,
                                                     const uint8_t* taken, float th, int* match_kp, int* n_matches) {
  return sim3p_core("cms_kfstore_search_by_projection_sim3", true, st, src, nsets, set_off, pos, normal, min_dist, max_dist, mp_desc, njobs, jobs, skip, taken, th, match_kp,
                    nullptr, n_matches);
}

extern "C" int cms_kfstore_fuse_search_sim3(cms_kfstore* st, cms_ctx* src, int nsets, const int* set_off, const float* pos, const float* normal, const float* min_dist,
                                            const float* max_dist, const uint8_t* mp_desc, int njobs, const cms_sim3_proj_job* jobs, const uint8_t* skip, float th,
                                            int* best_idx, int* best_dist) {
  return sim3p_core("cms_kfstore_fuse_search_sim3", false, st, src, nsets, set_off, pos, normal, min_dist, max_dist, mp_desc, njobs, jobs, skip, nullptr, th, best_idx, best_dist,
                    nullptr);
}

extern "C" int cms_sim3_proj_last_rounds(void) { return g_sim3p_last_rounds; }
