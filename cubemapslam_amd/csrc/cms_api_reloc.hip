// cms_api_reloc.hip -- host side of ORBMatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th,
// ORBdist) (src/ORBMatcher.cpp:253-378), the guided search Tracking::Relocalization runs twice per accepted PnP pose (Tracking.cpp:1101, :1115);
// included by cms_lib.hip after cms_api_bow.hip (cms_kfstore, cms_api_track.hip's helpers).  All jobs of a call are ONE launch sequence on the frame
// context's stream: one staged block up (the context's CmsStage), k_project_keyframe, the window query, k_search_local (one workgroup per job, no second-best test),
// k_rot_filter, one block back -- inside cms_retry_capacity like cms_search_by_projection.
#include <algorithm>
#include <cstring>
#include <vector>

namespace {
// st == NULL: the stand-alone entry (one job, slot unused, kf_angle[nmp] from the caller)
int reloc_run(cms_ctx* c, cms_kfstore* st, int njobs, const cms_kfproj_job* jobs, const float* kf_angle, float th, int orb_dist, int check_orientation,
              int* n_matches, const char* who) {
  const int kp_cap = c->g.kp_cap;
  std::vector<int> mp_off((size_t)njobs + 1, 0);
  for (int j = 0; j < njobs; ++j) mp_off[(size_t)j + 1] = mp_off[(size_t)j] + jobs[j].nmp;
  const int n = mp_off[(size_t)njobs];
  for (int j = 0; j < njobs; ++j) n_matches[j] = 0;
  if (n == 0) return CMS_OK;
  if (c->g.nlevels > 16) return cms_fail(CMS_ERR_UNSUPPORTED, "SearchByProjection (key frame): more than 16 pyramid levels");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (st) {
    const int rc = kfstore_wait_puts(st, s, njobs, [&](int j) { return jobs[j].slot; });
    if (rc) return rc;
  }
  const size_t n4 = (size_t)n * 4, j4 = (size_t)njobs * 4, kp4 = (size_t)kp_cap * 4;
  CmsBlock blk;
  const size_t o_pose = blk.take(12 * j4), o_jframe = blk.take(j4), o_jkp0 = blk.take(j4), o_mpoff = blk.take(j4, 4), o_ptjob = blk.take(n4), o_feat = blk.take(n4),
               o_pos = blk.take(3 * n4), o_min = blk.take(n4), o_max = blk.take(n4), o_desc = blk.take((size_t)n * 32), o_kpmp = blk.take(njobs * kp4);
  const size_t in_bytes = blk.size;
  const size_t o_match = blk.take(n4), o_nm = blk.take(j4), o_tot = blk.take(16);
  const size_t out_begin = o_kpmp, out_end = blk.size;
  const size_t o_qf = blk.take(n4), o_qx = blk.take(n4), o_qy = blk.take(n4), o_qr = blk.take(n4), o_qmin = blk.take(n4), o_qmax = blk.take(n4), o_ang = blk.take(n4),
               o_cnt = blk.take(n4), o_off = blk.take(n4, 4);
  const size_t o_idx = blk.size;
  return cms_retry_capacity(64 * n + 1024, who, [&](int cap, int& tot) -> int {
    const size_t o_pd = o_idx + cms_align((size_t)cap * 4);
    int rc = c->stage.reserve(s, o_pd + cms_align((size_t)cap * 2), out_end);
    if (rc) return rc;
    uint8_t* p = c->stage.d;
    uint8_t* h = c->stage.h;
    std::memcpy(h + o_mpoff, mp_off.data(), j4 + 4);
    for (int j = 0; j < njobs; ++j) {
      const cms_kfproj_job& q = jobs[j];
      const size_t m0 = (size_t)mp_off[(size_t)j], m = (size_t)q.nmp;
      std::memcpy(h + o_pose + 48 * (size_t)j, q.pose12, 48);
      reinterpret_cast<int*>(h + o_jframe)[j] = q.b;
      reinterpret_cast<int*>(h + o_jkp0)[j] = st ? st->h_kf[(size_t)q.slot].f0 : -1;
      int* km = reinterpret_cast<int*>(h + o_kpmp) + (size_t)j * kp_cap;
      for (int k = 0; k < kp_cap; ++k) km[k] = k < q.n ? q.kp_mp[k] : -1;
      if (m == 0) continue;
      int* pj = reinterpret_cast<int*>(h + o_ptjob) + m0;
      for (size_t k = 0; k < m; ++k) pj[k] = j;
      std::memcpy(h + o_feat + 4 * m0, st ? (const void*)q.kf_feat : (const void*)kf_angle, 4 * m);      // feature indices, or the angles themselves
      std::memcpy(h + o_pos + 12 * m0, q.pos, 12 * m); std::memcpy(h + o_min + 4 * m0, q.min_dist, 4 * m); std::memcpy(h + o_max + 4 * m0, q.max_dist, 4 * m);
      std::memcpy(h + o_desc + 32 * m0, q.mp_desc, 32 * m);
    }
    rc = c->stage.up(s, in_bytes, who);
    if (rc) return rc;
    CmsProjectKfArgs a = {};
    a.n = n; a.pt_job = (const int*)(p + o_ptjob); a.pose12 = (const float*)(p + o_pose); a.job_frame = (const int*)(p + o_jframe); a.job_kp0 = (const int*)(p + o_jkp0);
    a.kf_kp = st ? st->d_kp : nullptr; a.kf_feat = (const int*)(p + o_feat); a.kf_angle = (const float*)(p + o_feat);
    a.pos = (const float*)(p + o_pos); a.min_dist = (const float*)(p + o_min); a.max_dist = (const float*)(p + o_max);
    a.th = th; a.cos_fov = cms_cos_fov(c); a.log_scale = cms_log_scale(c); a.nlevels = c->g.nlevels; a.F = c->g.F;
    a.bounds_scaled = c->dist_bounds_scaled;
    cms_level_table(a.sf, c, c->scale, 0.0f);
    a.q_frame = (int*)(p + o_qf); a.qx = (float*)(p + o_qx); a.qy = (float*)(p + o_qy); a.qr = (float*)(p + o_qr); a.qmin = (int*)(p + o_qmin); a.qmax = (int*)(p + o_qmax);
    a.angle = (float*)(p + o_ang);
    hipLaunchKernelGGL(k_project_keyframe, dim3((n + 255) / 256), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    rc = cms_features_in_area_batch_device(c, n, p + o_qf, p + o_qx, p + o_qy, p + o_qr, p + o_qmin, p + o_qmax, p + o_cnt, p + o_off, p + o_idx, cap, p + o_tot);
    if (rc) return rc;
    CmsSearchLocalArgs g = track_search_local_args(c, p + o_mpoff, p + o_desc, p + o_off, p + o_idx, p + o_pd, (int*)(p + o_kpmp), p + o_match, nullptr, -1.0f, orb_dist, 0,
                                                   p + o_tot, cap);
    g.wg_frame = (const int*)(p + o_jframe);
    hipLaunchKernelGGL(k_search_local, dim3(njobs), dim3(1024), 0, s, g);
    CmsRotFilterArgs r = {};
    r.mp_off = g.mp_off; r.last_angle = (const float*)(p + o_ang); r.kp = g.kp; r.kp_mp = g.kp_mp; r.mp_match = g.mp_match; r.n_matches = (int*)(p + o_nm);
    r.check_orientation = check_orientation; r.total = g.total; r.cap = cap; r.wg_frame = g.wg_frame; r.kp_cap = kp_cap;
    hipLaunchKernelGGL(k_rot_filter, dim3(njobs), dim3(1024), 0, s, r);
    HIPCHK(hipGetLastError());
    rc = c->stage.back_and_wait(s, out_begin, out_end, who);
    if (rc) return rc;
    tot = *reinterpret_cast<const int*>(h + o_tot);
    if (tot > cap) return CMS_OK;
    for (int j = 0; j < njobs; ++j) {
      const cms_kfproj_job& q = jobs[j];
      if (q.nmp == 0) continue;                                        // kp_mp stays as the caller left it
      const int* km = reinterpret_cast<const int*>(h + o_kpmp) + (size_t)j * kp_cap;
      const int* rows = reinterpret_cast<const int*>(h + o_match) + mp_off[(size_t)j];
      if (q.n > 0) std::memcpy(q.kp_mp, km, (size_t)q.n * 4);
      track_rows_to_frame(c, q.b, q.nmp, rows, q.match);
      // the device stored the point's place in the whole call's list.  (A caller whose n is below the row's key-point count has left the rest of the
      // row free: a match there is reported, but kp_mp holds n entries only)
      for (int k = 0; k < q.nmp; ++k) if (q.match[k] >= 0 && q.match[k] < q.n) q.kp_mp[q.match[k]] = k;
      n_matches[j] = reinterpret_cast<const int*>(h + o_nm)[j];
    }
    return CMS_OK;
  });
}
// what both entries ask of a job's frame side and lists (the slot is the resident entry's business)
int reloc_check_job(const cms_ctx* c, const cms_kfproj_job& q, const char* who) {
  if (q.b < 0 || q.b >= c->area_frames) return cms_fail(CMS_ERR_ARG, (std::string(who) + ": no grid for this frame (cms_area_grid first)").c_str());
  if (q.n < 0 || q.n > c->g.kp_cap || q.nmp < 0 || (q.n > 0 && !q.kp_mp) || (q.nmp > 0 && (!q.pos || !q.min_dist || !q.max_dist || !q.mp_desc || !q.match)))
    return cms_fail(CMS_ERR_ARG, (std::string(who) + ": bad argument").c_str());
  return CMS_OK;
}
}  // namespace

extern "C" int cms_kfstore_search_by_projection(cms_kfstore* st, cms_ctx* src, int njobs, const cms_kfproj_job* jobs, float th, int orb_dist, int check_orientation,
                                                int* n_matches) {
  const char* who = "cms_kfstore_search_by_projection";
  if (!st || !src || njobs < 0 || (njobs > 0 && (!jobs || !n_matches))) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_projection: bad argument");
  if (njobs == 0) return CMS_OK;
  if (src->device != st->c->device) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_projection: the frame context and the store must share the device");
  if (src->g.kp_cap > CMS_TRACK_KPMAX) return cms_fail(CMS_ERR_UNSUPPORTED, "cms_kfstore_search_by_projection: more than 4096 key points per frame");
  std::vector<uint8_t> row_named((size_t)std::max(src->area_frames, 1), 0);
  for (int j = 0; j < njobs; ++j) {
    const cms_kfproj_job& q = jobs[j];
    if (q.slot < 0 || q.slot >= st->maxkf || !st->used[(size_t)q.slot]) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_projection: empty slot");
    const int rc = reloc_check_job(src, q, who);
    if (rc) return rc;
    // the reference's second call sees the first one's matches (and another pose): two jobs on one frame row cannot be one launch
    if (row_named[(size_t)q.b]) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_projection: two jobs name the same frame row");
    row_named[(size_t)q.b] = 1;
    if (q.nmp > 0 && !q.kf_feat) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_projection: bad argument");
    const int kn = st->h_kf[(size_t)q.slot].n;
    for (int k = 0; k < q.nmp; ++k) {
      if (q.kf_feat[k] < 0 || q.kf_feat[k] >= kn) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_projection: key-frame feature index out of range");
      if (k > 0 && q.kf_feat[k] <= q.kf_feat[k - 1]) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_projection: key-frame feature indices must ascend");
    }
  }
  return reloc_run(src, st, njobs, jobs, nullptr, th, orb_dist, check_orientation, n_matches, who);
}

extern "C" int cms_search_by_projection_keyframe(cms_ctx* c, int b, const float* pose12, int nmp, const float* kf_angle, const float* pos, const float* min_dist,
                                                 const float* max_dist, const uint8_t* mp_desc, float th, int orb_dist, int check_orientation, int nkp, int* kp_mp,
                                                 int* match, int* n_matches) {
  const char* who = "cms_search_by_projection_keyframe";
  if (!c || !pose12 || (nmp > 0 && !kf_angle)) return cms_fail(CMS_ERR_ARG, "cms_search_by_projection_keyframe: bad argument");
  if (c->g.kp_cap > CMS_TRACK_KPMAX) return cms_fail(CMS_ERR_UNSUPPORTED, "cms_search_by_projection_keyframe: more than 4096 key points per frame");
  cms_kfproj_job q = {};
  q.slot = -1; q.b = b; q.n = nkp; std::memcpy(q.pose12, pose12, 48); q.nmp = nmp; q.pos = pos; q.min_dist = min_dist; q.max_dist = max_dist; q.mp_desc = mp_desc; q.kp_mp = kp_mp; q.match = match;
  const int rc = reloc_check_job(c, q, who);
  if (rc) return rc;
  int nm = 0;
  const int rr = reloc_run(c, nullptr, 1, &q, kf_angle, th, orb_dist, check_orientation, &nm, who);
  if (n_matches) *n_matches = nm;
  return rr;
}
