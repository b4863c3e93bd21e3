// cms_api_ba_window.hip -- host side of cms_covis_local_ba_windows: the local BA windows of a group of key frames, assembled on the device from the
// observation index, the store's slots and the map-point table (csrc/cms_ba_window_core.h states the rules).  Included by cms_lib.hip behind
// cms_api_mappoints.hip (cms_covis, cms_mpstore) and cms_ba_window_kernels.hip.  Everything about the jobs that the host can know is checked before
// anything is enqueued; then one upload, four launches, one copy back and one wait on the store's stream (CmsStage of the index).  Outputs that all lie
// in pinned host memory are stored by the kernels themselves; only the counts and the missing-row flags come back through the stage.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

static int baw_fail(const char* why) { return cms_fail(CMS_ERR_ARG, (std::string("cms_covis_local_ba_windows: ") + why).c_str()); }

extern "C" int cms_covis_local_ba_windows(cms_covis* cv, cms_mpstore* mp, int njobs, const cms_ba_window_job* jobs, int cap_kf, int cap_points, int cap_edges,
                                          cms_ba_window_counts* counts, int* kf_member, int* point_id, double* poses, uint8_t* fixed, double* points, int* e_pose,
                                          int* e_point, double* e_obs, double* e_invsig2, int8_t* e_face, int* e_feat) {
  if (!cv || !mp || njobs < 0 || (njobs > 0 && !jobs)) return baw_fail("bad argument");
  if (cv->st != mp->st) return baw_fail("the index and the table belong to different stores");
  if (cap_kf < 1 || cap_points < 1 || cap_edges < 1) return baw_fail("a cap below 1");
  if (njobs == 0) return CMS_OK;
  if (!counts || !kf_member || !point_id || !poses || !fixed || !points || !e_pose || !e_point || !e_obs || !e_invsig2 || !e_face || !e_feat) return baw_fail("a null output array");
  std::lock_guard<std::mutex> lk(mp->mu);
  std::lock_guard<std::mutex> lkc(cv->mu);
  int rc = covis_ready(cv, "cms_covis_local_ba_windows");
  if (rc) return rc;
  cms_kfstore* st = cv->st;
  cms_ctx* c = st->c;
  if (c->g.nlevels > 16) return cms_fail(CMS_ERR_UNSUPPORTED, "cms_covis_local_ba_windows: more than 16 pyramid levels");
  const size_t M = (size_t)cv->M, Q = (size_t)njobs;
  // the jobs, and per job the features of its local rows: the bound of its local points
  static thread_local std::vector<int> seen, off, members, firsts;
  seen.assign(M, -1); off.assign(Q + 1, 0); members.clear(); firsts.resize(Q);
  size_t pid_stride = 1;
  for (int j = 0; j < njobs; ++j) {
    const cms_ba_window_job& J = jobs[j];
    if (J.n_local < 1 || !J.local_members) return baw_fail("a job without a local key frame (n_local < 1)");
    if (J.first_member < -1 || J.first_member >= cv->M) return baw_fail("first_member names no member");
    for (int k = 0; k < J.n_local; ++k) {
      const int m = J.local_members[k];
      if (m < 0 || m >= cv->M) return baw_fail("a job names no member");
      if (seen[(size_t)m] == j) return baw_fail("a job names a member twice");
      seen[(size_t)m] = j;
      members.push_back(m);
    }
    off[(size_t)j + 1] = (int)members.size();
    firsts[(size_t)j] = J.first_member;
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(kfstore_order_behind_puts(st));
  hipStream_t s = c->stream;
  HIPCHK(hipStreamWaitEvent(s, cv->built_ev, 0));
  const size_t T = members.size();
  for (int j = 0; j < njobs; ++j) {
    size_t sum = 0;
    for (int q = off[(size_t)j]; q < off[(size_t)j + 1]; ++q) sum += (size_t)cv->h_n[(size_t)members[(size_t)q]];
    pid_stride = std::max(pid_stride, sum);
  }
  const bool direct = cms_is_pinned(kf_member) && cms_is_pinned(point_id) && cms_is_pinned(poses) && cms_is_pinned(fixed) && cms_is_pinned(points) && cms_is_pinned(e_pose) &&
                      cms_is_pinned(e_point) && cms_is_pinned(e_obs) && cms_is_pinned(e_invsig2) && cms_is_pinned(e_face) && cms_is_pinned(e_feat);
  const size_t ck = (size_t)cap_kf, cp = (size_t)cap_points, ce = (size_t)cap_edges;
  CmsBlock blk;
  const size_t o_off = blk.take(4 * (Q + 1)), o_mem = blk.take(4 * T), o_first = blk.take(4 * Q), o_miss = blk.take(4 * Q), in_bytes = blk.size;
  const size_t o_cnt = blk.take(sizeof(cms_ba_window_counts) * Q), status_end = blk.size;
  size_t o_kfm = 0, o_pid = 0, o_pose = 0, o_fix = 0, o_pts = 0, o_ep = 0, o_eq = 0, o_eo = 0, o_ei = 0, o_ef = 0, o_et = 0;
  if (!direct) {
    o_kfm = blk.take(4 * Q * ck); o_pid = blk.take(4 * Q * cp); o_pose = blk.take(56 * Q * ck); o_fix = blk.take(Q * ck); o_pts = blk.take(24 * Q * cp);
    o_ep = blk.take(4 * Q * ce); o_eq = blk.take(4 * Q * ce); o_eo = blk.take(16 * Q * ce); o_ei = blk.take(8 * Q * ce); o_ef = blk.take(Q * ce); o_et = blk.take(4 * Q * ce);
  }
  const size_t host_bytes = blk.size;
  const size_t o_spid = blk.take(4 * Q * pid_stride), o_snp = blk.take(4 * Q), o_sec = blk.take(4 * Q * pid_stride), o_seo = blk.take(4 * Q * pid_stride), o_swi = blk.take(4 * Q * M);
  rc = cv->stage.reserve(s, blk.size, host_bytes);
  if (rc) return rc;
  uint8_t* h = cv->stage.h;
  uint8_t* d = cv->stage.d;
  std::memcpy(h + o_off, off.data(), 4 * (Q + 1)); std::memcpy(h + o_mem, members.data(), 4 * T); std::memcpy(h + o_first, firsts.data(), 4 * Q);
  std::memset(h + o_miss, 0, 4 * Q);
  rc = cv->stage.up(s, in_bytes, "cms_covis_local_ba_windows");
  if (rc) return rc;
  CmsBawArgs a;
  a.d = covis_dev(cv); a.kf = st->d_kf; a.st_kp = st->d_kp; a.st_rays = st->d_rays; a.st_maxf = st->maxf; a.t = mp->t;
  a.njobs = njobs; a.F = c->g.F; a.cos_fov = cms_cos_fov(c);
  cms_level_table(a.inv_sigma2, c, c->inv_sigma2, 0.0f);
  a.loc_off = (const int*)(d + o_off); a.loc_members = (const int*)(d + o_mem); a.first_member = (const int*)(d + o_first);
  a.cap_kf = cap_kf; a.cap_points = cap_points; a.cap_edges = cap_edges;
  a.pid_stride = (int)pid_stride; a.pid = (const int*)(d + o_spid); a.npts = (const int*)(d + o_snp); a.ecount = (int*)(d + o_sec); a.eoff = (int*)(d + o_seo); a.widx = (int*)(d + o_swi);
  a.missing = (int*)(d + o_miss); a.counts = (CmsBaWindowCounts*)(d + o_cnt);
  a.kf_member = direct ? kf_member : (int*)(d + o_kfm); a.point_id = direct ? point_id : (int*)(d + o_pid); a.poses = direct ? poses : (double*)(d + o_pose);
  a.fixed = direct ? fixed : d + o_fix; a.points = direct ? points : (double*)(d + o_pts); a.e_pose = direct ? e_pose : (int*)(d + o_ep);
  a.e_point = direct ? e_point : (int*)(d + o_eq); a.e_obs = direct ? e_obs : (double*)(d + o_eo); a.e_invsig2 = direct ? e_invsig2 : (double*)(d + o_ei);
  a.e_face = direct ? e_face : (int8_t*)(d + o_ef); a.e_feat = direct ? e_feat : (int*)(d + o_et);
  static bool lds_points[64] = {}, lds_frames[64] = {};
  if ((rc = covis_lds((const void*)k_covis_local_points, c->device, lds_points))) return rc;
  if ((rc = covis_lds((const void*)k_baw_frames, c->device, lds_frames))) return rc;
  const dim3 grid((unsigned)((pid_stride + 255) / 256), (unsigned)njobs);
  hipLaunchKernelGGL(k_covis_local_points, dim3((unsigned)njobs), dim3(1024), 4 * M, s, a.d, a.loc_off, a.loc_members, (int)pid_stride, (int*)(d + o_spid), (int*)(d + o_snp));
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_baw_count, grid, dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_baw_frames, dim3((unsigned)njobs), dim3(1024), 8 * M, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_baw_fill, grid, dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  rc = cv->stage.back_and_wait(s, o_miss, direct ? status_end : host_bytes, "cms_covis_local_ba_windows");
  if (rc) return rc;
  const int* miss = reinterpret_cast<const int*>(h + o_miss);
  for (int j = 0; j < njobs; ++j)
    if (miss[j]) return baw_fail(("job " + std::to_string(j) + ": a local point has no position in the table (list position " + std::to_string(miss[j] - 1) + ")").c_str());
  const cms_ba_window_counts* hc = reinterpret_cast<const cms_ba_window_counts*>(h + o_cnt);
  bool overflow = false;
  for (size_t j = 0; j < Q; ++j) {
    counts[j] = hc[j];
    overflow = overflow || hc[j].K > cap_kf || hc[j].P > cap_points || hc[j].E > cap_edges;
    if (direct) continue;
    const size_t k = (size_t)std::min(hc[j].K, cap_kf), p = (size_t)std::min(hc[j].P, cap_points), e = (size_t)std::min(hc[j].E, cap_edges);
    std::memcpy(kf_member + j * ck, h + o_kfm + 4 * j * ck, 4 * k); std::memcpy(poses + 7 * j * ck, h + o_pose + 56 * j * ck, 56 * k); std::memcpy(fixed + j * ck, h + o_fix + j * ck, k);
    std::memcpy(point_id + j * cp, h + o_pid + 4 * j * cp, 4 * p); std::memcpy(points + 3 * j * cp, h + o_pts + 24 * j * cp, 24 * p);
    std::memcpy(e_pose + j * ce, h + o_ep + 4 * j * ce, 4 * e); std::memcpy(e_point + j * ce, h + o_eq + 4 * j * ce, 4 * e); std::memcpy(e_obs + 2 * j * ce, h + o_eo + 16 * j * ce, 16 * e);
    std::memcpy(e_invsig2 + j * ce, h + o_ei + 8 * j * ce, 8 * e); std::memcpy(e_face + j * ce, h + o_ef + j * ce, e); std::memcpy(e_feat + j * ce, h + o_et + 4 * j * ce, 4 * e);
  }
  if (overflow) return cms_fail(CMS_ERR_OVERFLOW, "cms_covis_local_ba_windows: a job has more key frames, points or edges than its cap (counts says how many)");
  return CMS_OK;
}
