// cms_api_mpstats.hip -- host side of the map-point statistics: the table's counter columns (cms_mpstore_set_stats / add_stats / fetch_stats), the
// per-frame counting of Tracking (cms_mpstore_count), LocalMapping::MapPointCulling (cms_mpstore_culling), KeyFrame::TrackedMapPoints
// (cms_covis_tracked_map_points) and KeyFrame::ComputeSceneMedianDepth (cms_kfstore_scene_median_depth).  Included by cms_lib.hip behind
// cms_api_mappoints.hip (cms_mpstore, mpstore_records) and cms_mpstats_kernels.hip.  Every entry checks all its arguments before anything is
// enqueued: a refused call writes nothing.
//
// Streams.  The counters are written from two sides: set / add / erase / culling on the store's stream, cms_mpstore_count on the FRAME context's
// stream.  A counting call makes its stream wait for the table's last write (write_ev) and records an event per frame context; every entry on the
// store's stream that reads or resets the counters waits for those events first (mpstore_behind_counts, which mpstore_records calls too).
//
// cms_mpstore_count is asynchronous, so its ids and flags cannot travel through the table's staging block: the next call on the handle would
// refill the pinned half while the copy is still on its way.  They go through a pinned ring of four blocks the kernel reads itself, the pattern of
// cms_mpstore_set's records; a block is rewritten four calls later, behind the event of the kernel that read it.

static int mpstats_check_off(const char* who, int njobs, const int* off) {
  if (off[0] != 0) return mpstore_fail(who, "off must start at 0");
  for (int j = 0; j < njobs; ++j) if (off[j + 1] < off[j]) return mpstore_fail(who, "off must not descend");
  return CMS_OK;
}

static int mpstore_stats_records(cms_mpstore* mp, const char* who, int n, const int* ids, int flags, const int* first_kf, const int* visible, const int* found) {
  if (const char* why = mpstore_check_ids(mp, n, ids, true)) return mpstore_fail(who, why);
  for (int i = 0; i < n; ++i) if (!(mp->state[(size_t)ids[i]] & CMS_MP_ROW_SET)) return mpstore_fail(who, "a row that was never set (or was erased)");
  if (!flags) return CMS_OK;
  return mpstore_records(mp, n, [&](int* rec) {
    for (int i = 0; i < n; ++i) {
      int* r = rec + 6 * (size_t)i;
      r[0] = ids[i]; r[1] = flags; r[2] = first_kf ? first_kf[i] : 0; r[3] = visible ? visible[i] : 0; r[4] = found ? found[i] : 0; r[5] = -1;
    }
  });
}

extern "C" int cms_mpstore_set_stats(cms_mpstore* mp, int n, const int* ids, const int* first_kf, const int* visible, const int* found) {
  if (!mp || n < 0 || (n > 0 && !ids)) return cms_fail(CMS_ERR_ARG, "cms_mpstore_set_stats: bad argument");
  if (n == 0) return CMS_OK;
  for (int i = 0; i < n; ++i)
    if ((first_kf && first_kf[i] < -1) || (visible && visible[i] < 1) || (found && found[i] < 0))
      return cms_fail(CMS_ERR_ARG, "cms_mpstore_set_stats: first_kf >= -1, visible >= 1, found >= 0");
  std::lock_guard<std::mutex> lk(mp->mu);
  const int flags = (first_kf ? CMS_MP_REC_FIRST_KF : 0) | (visible ? CMS_MP_REC_VISIBLE : 0) | (found ? CMS_MP_REC_FOUND : 0);
  return mpstore_stats_records(mp, "cms_mpstore_set_stats", n, ids, flags, first_kf, visible, found);
}

extern "C" int cms_mpstore_add_stats(cms_mpstore* mp, int n, const int* ids, const int* d_visible, const int* d_found) {
  if (!mp || n < 0 || (n > 0 && !ids)) return cms_fail(CMS_ERR_ARG, "cms_mpstore_add_stats: bad argument");
  if (n == 0) return CMS_OK;
  for (int i = 0; i < n; ++i)
    if ((d_visible && d_visible[i] < 0) || (d_found && d_found[i] < 0)) return cms_fail(CMS_ERR_ARG, "cms_mpstore_add_stats: a negative amount");
  std::lock_guard<std::mutex> lk(mp->mu);
  const int flags = (d_visible ? CMS_MP_REC_VISIBLE : 0) | (d_found ? CMS_MP_REC_FOUND : 0);
  return mpstore_stats_records(mp, "cms_mpstore_add_stats", n, ids, flags ? flags | CMS_MP_REC_ADD : 0, nullptr, d_visible, d_found);
}

extern "C" int cms_mpstore_fetch_stats(cms_mpstore* mp, int n, const int* ids, int* visible, int* found, int* first_kf) {
  if (!mp || n < 0 || (n > 0 && !ids)) return cms_fail(CMS_ERR_ARG, "cms_mpstore_fetch_stats: bad argument");
  if (n == 0) return CMS_OK;
  std::lock_guard<std::mutex> lk(mp->mu);
  if (const char* why = mpstore_check_ids(mp, n, ids, false)) return mpstore_fail("cms_mpstore_fetch_stats", why);
  cms_ctx* c = mp->st->c;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  HIPCHK(mpstore_behind_counts(mp, s));
  const size_t n4 = 4 * (size_t)n;
  CmsBlock blk;
  const size_t o_ids = blk.take(n4), in_bytes = blk.size, o_vis = blk.take(n4), o_found = blk.take(n4), o_first = blk.take(n4);
  int rc = mp->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = mp->stage.h;
  uint8_t* d = mp->stage.d;
  std::memcpy(h + o_ids, ids, n4);
  rc = mp->stage.up(s, in_bytes, "cms_mpstore_fetch_stats");
  if (rc) return rc;
  hipLaunchKernelGGL(k_mp_gather_stats, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mp->t, n, (const int*)(d + o_ids), (int*)(d + o_vis), (int*)(d + o_found),
                     (int*)(d + o_first));
  HIPCHK(hipGetLastError());
  rc = mp->stage.back_and_wait(s, o_vis, blk.size, "cms_mpstore_fetch_stats");
  if (rc) return rc;
  if (visible) std::memcpy(visible, h + o_vis, n4);
  if (found) std::memcpy(found, h + o_found, n4);
  if (first_kf) std::memcpy(first_kf, h + o_first, n4);
  return CMS_OK;
}

extern "C" int cms_mpstore_count(cms_mpstore* mp, cms_ctx* src, int which, int njobs, const int* off, const int* ids, const uint8_t* flag, int count_if) {
  if (!mp || !src || njobs < 0 || (njobs > 0 && !off) || (which != CMS_MP_VISIBLE && which != CMS_MP_FOUND)) return cms_fail(CMS_ERR_ARG, "cms_mpstore_count: bad argument");
  if (src->device != mp->st->c->device) return cms_fail(CMS_ERR_ARG, "cms_mpstore_count: the frame context and the store must share the device");
  if (njobs == 0) return CMS_OK;
  int rc = mpstats_check_off("cms_mpstore_count", njobs, off);
  if (rc) return rc;
  const size_t T = (size_t)off[njobs];
  if (T == 0) return CMS_OK;
  if (!ids) return cms_fail(CMS_ERR_ARG, "cms_mpstore_count: bad argument");
  std::lock_guard<std::mutex> lk(mp->mu);
  for (size_t i = 0; i < T; ++i) {
    const int id = ids[i];
    if (id < -1 || id >= mp->t.max_points) return mpstore_fail("cms_mpstore_count", "an id outside the table");
    if (id < 0 || (flag && (flag[i] != 0) != (count_if != 0))) continue;
    if (!(mp->state[(size_t)id] & CMS_MP_ROW_SET)) return mpstore_fail("cms_mpstore_count", "a counted row that was never set (or was erased)");
  }
  HIPCHK(hipSetDevice(src->device));
  hipStream_t s = src->stream;
  // the block of the ring: T ids, then T flags
  const unsigned ring = mp->cnt_call++ & 3;
  if (!mp->cnt_ev[ring]) HIPCHK(hipEventCreateWithFlags(&mp->cnt_ev[ring], hipEventDisableTiming));
  if (mp->cnt_ev_set[ring]) HIPCHK(hipEventSynchronize(mp->cnt_ev[ring]));      // the kernel that last read this block: four calls ago
  const size_t bytes = 4 * T + (flag ? T : 0);
  if (mp->cnt_cap[ring] < bytes) {
    if (mp->h_cnt[ring]) { HIPCHK(hipHostFree(mp->h_cnt[ring])); mp->h_cnt[ring] = nullptr; mp->cnt_cap[ring] = 0; }
    const size_t want = bytes + bytes / 2 + 1024;
    // non-coherent: the kernel that reads the block is launched after it is filled, and a launch makes the host's writes visible to it.  (Measured
    // the same as a coherent block, profiles/mpstats.md: the call's 1.1 ms at 256 frames x 1 500 ids is the checking pass above.)
    HIPCHK(hipHostMalloc((void**)&mp->h_cnt[ring], want, hipHostMallocMapped | hipHostMallocNonCoherent));
    mp->cnt_cap[ring] = want;
  }
  uint8_t* blk = mp->h_cnt[ring];
  std::memcpy(blk, ids, 4 * T);
  if (flag) std::memcpy(blk + 4 * T, flag, T);
  if (mp->written) HIPCHK(hipStreamWaitEvent(s, mp->write_ev, 0));      // the table's last write ran on the store's stream
  hipLaunchKernelGGL(k_mp_count, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, which == CMS_MP_VISIBLE ? mp->t.visible : mp->t.found, mp->t.max_points,
                     (const int*)blk, flag ? (const uint8_t*)(blk + 4 * T) : nullptr, count_if, (int)T);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(mp->cnt_ev[ring], s));
  mp->cnt_ev_set[ring] = true;
  // the event the store's stream waits for: one per frame context, so that two contexts' calls are both covered
  hipEvent_t* done = nullptr;
  for (auto& e : mp->count_done) if (e.first == src) done = &e.second;
  if (!done) {
    // contexts come and go and the handle cannot see them leave: beyond 16 the oldest entry is waited for (its context's last count, long
    // through) and dropped, so the list and the waits of mpstore_behind_counts stay bounded
    if (mp->count_done.size() >= 16) {
      HIPCHK(hipEventSynchronize(mp->count_done.front().second));
      (void)hipEventDestroy(mp->count_done.front().second);
      mp->count_done.erase(mp->count_done.begin());
    }
    hipEvent_t ev = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    mp->count_done.emplace_back(src, ev);
    done = &mp->count_done.back().second;
  }
  HIPCHK(hipEventRecord(*done, s));
  return CMS_OK;
}

extern "C" int cms_mpstore_culling(cms_mpstore* mp, cms_covis* cv, int njobs, const int* off, const int* ids, const int* current_kf, int th_obs, int apply,
                                   uint8_t* verdict) {
  if (!mp || !cv || njobs < 0 || th_obs < 0 || (njobs > 0 && (!off || !current_kf))) return cms_fail(CMS_ERR_ARG, "cms_mpstore_culling: bad argument");
  if (cv->st != mp->st) return cms_fail(CMS_ERR_ARG, "cms_mpstore_culling: the index belongs to another store");
  std::lock_guard<std::mutex> lk(mp->mu);
  std::lock_guard<std::mutex> lkc(cv->mu);
  int rc = covis_ready(cv, "cms_mpstore_culling");
  if (rc) return rc;
  if (njobs == 0) return CMS_OK;
  rc = mpstats_check_off("cms_mpstore_culling", njobs, off);
  if (rc) return rc;
  const int n = off[njobs];
  if (n == 0) return CMS_OK;
  if (!ids || !verdict) return cms_fail(CMS_ERR_ARG, "cms_mpstore_culling: bad argument");
  if (const char* why = mpstore_check_ids(mp, n, ids, true)) return mpstore_fail("cms_mpstore_culling", why);
  cms_kfstore* st = mp->st;
  cms_ctx* c = st->c;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(kfstore_order_behind_puts(st));
  hipStream_t s = c->stream;
  HIPCHK(hipStreamWaitEvent(s, cv->built_ev, 0));
  HIPCHK(mpstore_behind_counts(mp, s));
  const size_t Q = (size_t)njobs;
  CmsBlock blk;
  const size_t o_off = blk.take(4 * (Q + 1)), o_cur = blk.take(4 * Q), o_ids = blk.take(4 * (size_t)n), in_bytes = blk.size, o_v = blk.take((size_t)n);
  rc = mp->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = mp->stage.h;
  uint8_t* d = mp->stage.d;
  std::memcpy(h + o_off, off, 4 * (Q + 1)); std::memcpy(h + o_cur, current_kf, 4 * Q); std::memcpy(h + o_ids, ids, 4 * (size_t)n);
  rc = mp->stage.up(s, in_bytes, "cms_mpstore_culling");
  if (rc) return rc;
  CmsMpCulling a;
  a.d = covis_dev(cv); a.t = mp->t; a.st_mp = st->d_mp; a.st_maxf = st->maxf;
  a.njobs = njobs; a.n = n; a.off = (const int*)(d + o_off); a.ids = (const int*)(d + o_ids); a.current_kf = (const int*)(d + o_cur);
  a.th_obs = th_obs; a.apply = apply ? 1 : 0; a.verdict = d + o_v;
  hipLaunchKernelGGL(k_mp_culling, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, a);      // four wavefronts, four ids
  HIPCHK(hipGetLastError());
  if (apply) { HIPCHK(hipEventRecord(mp->write_ev, s)); mp->written = true; }
  rc = mp->stage.back_and_wait(s, o_v, blk.size, "cms_mpstore_culling");
  if (rc) return rc;
  std::memcpy(verdict, h + o_v, (size_t)n);
  if (apply)
    for (int i = 0; i < n; ++i)
      if (verdict[i] == CMS_MP_BAD_RATIO || verdict[i] == CMS_MP_BAD_FEW_OBS) mp->state[(size_t)ids[i]] = 0;
  return CMS_OK;
}

extern "C" int cms_covis_tracked_map_points(cms_covis* cv, cms_ctx* src, int njobs, const int* job_member, const int* min_obs, int* count) {
  if (!cv || !src || njobs < 0 || (njobs > 0 && (!job_member || !min_obs || !count))) return cms_fail(CMS_ERR_ARG, "cms_covis_tracked_map_points: bad argument");
  if (njobs == 0) return CMS_OK;
  if (src->device != cv->st->c->device) return cms_fail(CMS_ERR_ARG, "cms_covis_tracked_map_points: the frame context and the store must share the device");
  std::lock_guard<std::mutex> lk(cv->mu);
  int rc = covis_ready(cv, "cms_covis_tracked_map_points");
  if (rc) return rc;
  for (int j = 0; j < njobs; ++j) if (job_member[j] < 0 || job_member[j] >= cv->M) return cms_fail(CMS_ERR_ARG, "cms_covis_tracked_map_points: a job names no member");
  HIPCHK(hipSetDevice(src->device));
  hipStream_t s = src->stream;
  HIPCHK(hipStreamWaitEvent(s, cv->built_ev, 0));
  const size_t Q = (size_t)njobs;
  CmsBlock blk;
  const size_t o_job = blk.take(4 * Q), o_min = blk.take(4 * Q), in_bytes = blk.size, o_cnt = blk.take(4 * Q);
  rc = cv->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = cv->stage.h;
  uint8_t* d = cv->stage.d;
  std::memcpy(h + o_job, job_member, 4 * Q); std::memcpy(h + o_min, min_obs, 4 * Q);
  rc = cv->stage.up(s, in_bytes, "cms_covis_tracked_map_points");
  if (rc) return rc;
  hipLaunchKernelGGL(k_covis_tracked, dim3((unsigned)((njobs + 3) / 4)), dim3(256), 0, s, covis_dev(cv), njobs, (const int*)(d + o_job), (const int*)(d + o_min), (int*)(d + o_cnt));
  HIPCHK(hipGetLastError());
  rc = cv->stage.back_and_wait(s, o_cnt, blk.size, "cms_covis_tracked_map_points");
  if (rc) return rc;
  std::memcpy(count, h + o_cnt, 4 * Q);
  return CMS_OK;
}

extern "C" int cms_kfstore_scene_median_depth(cms_kfstore* st, cms_mpstore* mp, int n, const int* slots, int q, int store, float* depth, int* n_depths) {
  if (!st || !mp || n < 0 || q < 1 || (n > 0 && (!slots || !depth || !n_depths))) return cms_fail(CMS_ERR_ARG, "cms_kfstore_scene_median_depth: bad argument");
  if (mp->st != st) return cms_fail(CMS_ERR_ARG, "cms_kfstore_scene_median_depth: the table belongs to another store");
  if (n == 0) return CMS_OK;
  int max_n = 0;
  {
    std::vector<uint8_t> seen((size_t)st->maxkf, 0);
    for (int i = 0; i < n; ++i) {
      const int s = slots[i];
      if (s < 0 || s >= st->maxkf || !st->used[(size_t)s]) return cms_fail(CMS_ERR_ARG, "cms_kfstore_scene_median_depth: a slot is empty");
      if (seen[(size_t)s]) return cms_fail(CMS_ERR_ARG, "cms_kfstore_scene_median_depth: a slot is named twice");
      seen[(size_t)s] = 1;
      max_n = std::max(max_n, std::min(st->h_kf[(size_t)s].n, st->maxf));
    }
  }
  std::lock_guard<std::mutex> lk(mp->mu);
  cms_ctx* c = st->c;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(kfstore_order_behind_puts(st));
  hipStream_t s = c->stream;      // pose updates, mp-row updates and the table's records all ran here: the stream orders the call behind them
  const size_t n4 = 4 * (size_t)n;
  CmsBlock blk;
  const size_t o_slots = blk.take(n4), in_bytes = blk.size, o_depth = blk.take(n4), o_nd = blk.take(n4);
  int rc = mp->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = mp->stage.h;
  uint8_t* d = mp->stage.d;
  std::memcpy(h + o_slots, slots, n4);
  rc = mp->stage.up(s, in_bytes, "cms_kfstore_scene_median_depth");
  if (rc) return rc;
  static bool lds_done[64] = {};
  rc = cms_lds_ceiling_once((const void*)k_kf_scene_median, 4 * (CMS_AREA_MAXKP + 4), c->device, lds_done);
  if (rc) return rc;
  CmsKfMedian a;
  a.kf = st->d_kf; a.st_mp = st->d_mp; a.st_maxf = st->maxf; a.t = mp->t; a.slots = (const int*)(d + o_slots); a.q = q; a.cap = max_n;
  a.depth = (float*)(d + o_depth); a.n_depths = (int*)(d + o_nd);
  hipLaunchKernelGGL(k_kf_scene_median, dim3((unsigned)n), dim3(256), 4 * ((size_t)max_n + 4), s, a);
  HIPCHK(hipGetLastError());
  rc = mp->stage.back_and_wait(s, o_depth, blk.size, "cms_kfstore_scene_median_depth");
  if (rc) return rc;
  std::memcpy(depth, h + o_depth, n4); std::memcpy(n_depths, h + o_nd, n4);
  if (store)
    for (int i = 0; i < n; ++i) if (n_depths[i] > 0) st->h_median[(size_t)slots[i]] = depth[i];
  return CMS_OK;
}
