// cms_api_mappoints.hip -- host side of the map-point table (cms_mpstore_*) and of the two consumers that take ids into it
// (cms_search_local_points_ids, cms_kfstore_fuse_search_sets_ids).  Included by cms_lib.hip behind cms_api_covis.hip (cms_covis) and
// cms_mappoint_kernels.hip.  A cms_mpstore belongs to ONE store: rows are indexed by the map point's id, the ids the store's mp rows and the index
// hold.  set / erase are one kernel reading a pinned ring block, asynchronous on the store's stream; refresh and fetch run there too and are
// synchronous (one upload, one launch, one copy back, one wait: CmsStage).  A host-side state byte per row lets every entry check all its
// arguments BEFORE anything is enqueued: a refused call writes nothing.  Calls on one handle are serialised by its mutex.
#include <algorithm>
#include <cstring>
#include <vector>

#define CMS_MP_ROW_SET 1
#define CMS_MP_ROW_DESC 2
#define CMS_MP_ROW_NORMAL 4

struct cms_mpstore {
  std::mutex mu;
  cms_kfstore* st = nullptr;
  CmsMpTable t = {};
  std::vector<uint8_t> state;               // per row: CMS_MP_ROW_*
  std::vector<uint8_t> seen;                // scratch of the duplicate check, all zero between calls
  // set / erase: a pinned ring of four record blocks (cms_kfstore_update_map_points' pattern)
  int* h_rec[4] = {nullptr, nullptr, nullptr, nullptr}; size_t rec_cap[4] = {0, 0, 0, 0};
  hipEvent_t rec_ev[4] = {nullptr, nullptr, nullptr, nullptr}; bool rec_ev_set[4] = {false, false, false, false};
  unsigned rec_call = 0;
  hipEvent_t write_ev = nullptr; bool written = false;      // behind the table's last write on the store's stream
  // cms_mpstore_count (cms_api_mpstats.hip): a pinned ring of four blocks of ids and flags, and per frame context the event behind its last call
  uint8_t* h_cnt[4] = {nullptr, nullptr, nullptr, nullptr}; size_t cnt_cap[4] = {0, 0, 0, 0};
  hipEvent_t cnt_ev[4] = {nullptr, nullptr, nullptr, nullptr}; bool cnt_ev_set[4] = {false, false, false, false};
  unsigned cnt_call = 0;
  std::vector<std::pair<cms_ctx*, hipEvent_t>> count_done;
  CmsStage stage;
};

extern "C" void cms_mpstore_destroy(cms_mpstore* mp) {
  if (!mp) return;
  if (mp->st && mp->st->c) (void)hipSetDevice(mp->st->c->device);
  void* bufs[] = {mp->t.pos, mp->t.normal, mp->t.min_dist, mp->t.max_dist, mp->t.desc, mp->t.ref, mp->t.best, mp->t.visible, mp->t.found, mp->t.first_kf};
  for (void* b : bufs) if (b) (void)hipFree(b);
  for (int i = 0; i < 4; ++i) { if (mp->h_cnt[i]) (void)hipHostFree(mp->h_cnt[i]); if (mp->cnt_ev[i]) (void)hipEventDestroy(mp->cnt_ev[i]); }
  for (auto& e : mp->count_done) (void)hipEventDestroy(e.second);
  for (int i = 0; i < 4; ++i) { if (mp->h_rec[i]) (void)hipHostFree(mp->h_rec[i]); if (mp->rec_ev[i]) (void)hipEventDestroy(mp->rec_ev[i]); }
  if (mp->write_ev) (void)hipEventDestroy(mp->write_ev);
  mp->stage.release();
  delete mp;
}
extern "C" int cms_mpstore_create(cms_mpstore** out, cms_kfstore* st, int max_points) {
  if (!out || !st || max_points < 1) return cms_fail(CMS_ERR_ARG, "cms_mpstore_create: bad argument");
  if (max_points > CMS_COVIS_MAX_ID) return cms_fail(CMS_ERR_ARG, "cms_mpstore_create: ids are below 2^30");
  if (st->c->g.nlevels > 16) return cms_fail(CMS_ERR_UNSUPPORTED, "cms_mpstore_create: more than 16 pyramid levels");
  HIPCHK(hipSetDevice(st->c->device));
  cms_mpstore* mp = new cms_mpstore();
  mp->st = st; mp->t.max_points = max_points;
  const size_t n = (size_t)max_points;
  hipStream_t s = st->c->stream;
  bool ok = hipEventCreateWithFlags(&mp->write_ev, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipMalloc((void**)&mp->t.pos, 12 * n) == hipSuccess && hipMalloc((void**)&mp->t.normal, 12 * n) == hipSuccess;
  ok = ok && hipMalloc((void**)&mp->t.min_dist, 4 * n) == hipSuccess && hipMalloc((void**)&mp->t.max_dist, 4 * n) == hipSuccess;
  ok = ok && hipMalloc((void**)&mp->t.desc, 32 * n) == hipSuccess && hipMalloc((void**)&mp->t.ref, 4 * n) == hipSuccess;
  ok = ok && hipMalloc((void**)&mp->t.best, 8 * n) == hipSuccess;
  ok = ok && hipMalloc((void**)&mp->t.visible, 4 * n) == hipSuccess && hipMalloc((void**)&mp->t.found, 4 * n) == hipSuccess && hipMalloc((void**)&mp->t.first_kf, 4 * n) == hipSuccess;
  // an empty row: zeros, no reference slot, no best observation (what k_mp_set's erase leaves)
  ok = ok && hipMemsetAsync(mp->t.pos, 0, 12 * n, s) == hipSuccess && hipMemsetAsync(mp->t.normal, 0, 12 * n, s) == hipSuccess;
  ok = ok && hipMemsetAsync(mp->t.min_dist, 0, 4 * n, s) == hipSuccess && hipMemsetAsync(mp->t.max_dist, 0, 4 * n, s) == hipSuccess;
  ok = ok && hipMemsetAsync(mp->t.desc, 0, 32 * n, s) == hipSuccess && hipMemsetAsync(mp->t.ref, 0xFF, 4 * n, s) == hipSuccess;
  ok = ok && hipMemsetAsync(mp->t.best, 0xFF, 8 * n, s) == hipSuccess;
  // (the counters of both MapPoint constructors: CMS_MP_EMPTY_*)
  ok = ok && hipMemsetD32Async((hipDeviceptr_t)mp->t.visible, CMS_MP_EMPTY_VISIBLE, n, s) == hipSuccess && hipMemsetD32Async((hipDeviceptr_t)mp->t.found, CMS_MP_EMPTY_FOUND, n, s) == hipSuccess;
  ok = ok && hipMemsetAsync(mp->t.first_kf, 0xFF, 4 * n, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  if (!ok) { cms_mpstore_destroy(mp); return cms_fail(CMS_ERR_HIP, "cms_mpstore_create: out of device memory"); }
  mp->state.assign(n, 0); mp->seen.assign(n, 0);
  *out = mp;
  return CMS_OK;
}

// every id inside the table, none named twice (twice = false: only the range).  NULL, or the reason
static const char* mpstore_check_ids(cms_mpstore* mp, int n, const int* ids, bool twice) {
  const char* why = nullptr;
  int marked = 0;
  for (; marked < n && !why; ++marked) {
    const int id = ids[marked];
    if (id < 0 || id >= mp->t.max_points) { why = "an id outside the table"; break; }
    if (twice) { if (mp->seen[(size_t)id]) { why = "an id is named twice"; break; } mp->seen[(size_t)id] = 1; }
  }
  if (twice) for (int i = 0; i < marked; ++i) mp->seen[(size_t)ids[i]] = 0;
  return why;
}
static int mpstore_fail(const char* who, const char* why) { return cms_fail(CMS_ERR_ARG, (std::string(who) + ": " + why).c_str()); }

// the stream waits (on the device) for every cms_mpstore_count enqueued so far: in front of whatever reads or resets the counters
static hipError_t mpstore_behind_counts(cms_mpstore* mp, hipStream_t s) {
  for (auto& e : mp->count_done) { const hipError_t rc = hipStreamWaitEvent(s, e.second, 0); if (rc != hipSuccess) return rc; }
  return hipSuccess;
}

// n records through the next ring block, one k_mp_set behind them; fill(rec) writes the 6 n words
template <class Fill>
static int mpstore_records(cms_mpstore* mp, int n, Fill&& fill) {
  cms_ctx* c = mp->st->c;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(kfstore_order_behind_puts(mp->st));
  HIPCHK(mpstore_behind_counts(mp, c->stream));
  const unsigned ring = mp->rec_call++ & 3;
  if (!mp->rec_ev[ring]) HIPCHK(hipEventCreateWithFlags(&mp->rec_ev[ring], hipEventDisableTiming));
  if (mp->rec_ev_set[ring]) HIPCHK(hipEventSynchronize(mp->rec_ev[ring]));      // the kernel that last read this block: four calls ago
  if (mp->rec_cap[ring] < (size_t)n) {
    if (mp->h_rec[ring]) { HIPCHK(hipHostFree(mp->h_rec[ring])); mp->h_rec[ring] = nullptr; mp->rec_cap[ring] = 0; }
    const size_t want = (size_t)n + (size_t)n / 2 + 256;
    HIPCHK(hipHostMalloc((void**)&mp->h_rec[ring], want * 24, hipHostMallocMapped | hipHostMallocCoherent));
    mp->rec_cap[ring] = want;
  }
  fill(mp->h_rec[ring]);
  hipLaunchKernelGGL(k_mp_set, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, mp->t, (const int*)mp->h_rec[ring], n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(mp->rec_ev[ring], c->stream));
  mp->rec_ev_set[ring] = true;
  HIPCHK(hipEventRecord(mp->write_ev, c->stream));
  mp->written = true;
  return CMS_OK;
}

extern "C" int cms_mpstore_set(cms_mpstore* mp, int n, const int* ids, const float* pos, const int* ref_slot) {
  if (!mp || n < 0 || (n > 0 && !ids)) return cms_fail(CMS_ERR_ARG, "cms_mpstore_set: bad argument");
  if (n == 0) return CMS_OK;
  std::lock_guard<std::mutex> lk(mp->mu);
  if (const char* why = mpstore_check_ids(mp, n, ids, true)) return mpstore_fail("cms_mpstore_set", why);
  for (int i = 0; i < n; ++i) {
    if (!(mp->state[(size_t)ids[i]] & CMS_MP_ROW_SET) && (!pos || !ref_slot)) return mpstore_fail("cms_mpstore_set", "a new row wants a position and a reference slot");
    if (ref_slot && (ref_slot[i] < 0 || ref_slot[i] >= mp->st->maxkf)) return mpstore_fail("cms_mpstore_set", "a reference slot outside the store");
  }
  const int flags = (pos ? CMS_MP_REC_POS : 0) | (ref_slot ? CMS_MP_REC_REF : 0);
  const int rc = mpstore_records(mp, n, [&](int* rec) {
    for (int i = 0; i < n; ++i) {
      int* r = rec + 6 * (size_t)i;
      r[0] = ids[i]; r[1] = flags; r[5] = ref_slot ? ref_slot[i] : -1;
      if (pos) std::memcpy(r + 2, pos + 3 * (size_t)i, 12); else r[2] = r[3] = r[4] = 0;
    }
  });
  if (rc) return rc;
  for (int i = 0; i < n; ++i) mp->state[(size_t)ids[i]] |= CMS_MP_ROW_SET;
  return CMS_OK;
}

extern "C" int cms_mpstore_erase(cms_mpstore* mp, int n, const int* ids) {
  if (!mp || n < 0 || (n > 0 && !ids)) return cms_fail(CMS_ERR_ARG, "cms_mpstore_erase: bad argument");
  if (n == 0) return CMS_OK;
  std::lock_guard<std::mutex> lk(mp->mu);
  if (const char* why = mpstore_check_ids(mp, n, ids, true)) return mpstore_fail("cms_mpstore_erase", why);
  const int rc = mpstore_records(mp, n, [&](int* rec) {
    for (int i = 0; i < n; ++i) { int* r = rec + 6 * (size_t)i; r[0] = ids[i]; r[1] = CMS_MP_REC_ERASE; r[2] = r[3] = r[4] = 0; r[5] = -1; }
  });
  if (rc) return rc;
  for (int i = 0; i < n; ++i) mp->state[(size_t)ids[i]] = 0;
  return CMS_OK;
}

extern "C" int cms_mpstore_refresh(cms_mpstore* mp, cms_covis* cv, int n, const int* ids, int what, uint8_t* status) {
  if (!mp || !cv || n < 0 || (n > 0 && (!ids || !status)) || what < 1 || what > (CMS_MP_DESCRIPTOR | CMS_MP_NORMAL_DEPTH))
    return cms_fail(CMS_ERR_ARG, "cms_mpstore_refresh: bad argument");
  if (cv->st != mp->st) return cms_fail(CMS_ERR_ARG, "cms_mpstore_refresh: the index belongs to another store");
  if (n == 0) return CMS_OK;
  std::lock_guard<std::mutex> lk(mp->mu);
  std::lock_guard<std::mutex> lkc(cv->mu);
  int rc = covis_ready(cv, "cms_mpstore_refresh");
  if (rc) return rc;
  if (const char* why = mpstore_check_ids(mp, n, ids, true)) return mpstore_fail("cms_mpstore_refresh", why);
  for (int i = 0; i < n; ++i) if (!(mp->state[(size_t)ids[i]] & CMS_MP_ROW_SET)) return mpstore_fail("cms_mpstore_refresh", "a row that was never set (or was erased)");
  if (cv->M == 0) { std::fill(status, status + n, (uint8_t)CMS_MP_NO_OBSERVATION); return CMS_OK; }      // an empty index knows no id
  cms_kfstore* st = mp->st;
  cms_ctx* c = st->c;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(kfstore_order_behind_puts(st));
  hipStream_t s = c->stream;
  HIPCHK(hipStreamWaitEvent(s, cv->built_ev, 0));
  CmsBlock blk;
  const size_t o_ids = blk.take(4 * (size_t)n), in_bytes = blk.size, o_st = blk.take((size_t)n);
  rc = mp->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = mp->stage.h;
  uint8_t* d = mp->stage.d;
  std::memcpy(h + o_ids, ids, 4 * (size_t)n);
  rc = mp->stage.up(s, in_bytes, "cms_mpstore_refresh");
  if (rc) return rc;
  CmsMpRefresh a;
  a.d = covis_dev(cv); a.kf = st->d_kf; a.st_desc = (const uint4*)st->d_desc; a.st_maxf = st->maxf; a.t = mp->t;
  a.n = n; a.ids = (const int*)(d + o_ids); a.what = what; a.nlevels = c->g.nlevels; a.status = d + o_st;
  cms_level_table(a.sf, c, c->scale, 1.0f);
  hipLaunchKernelGGL(k_mp_refresh, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, a);      // four wavefronts, four map points
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(mp->write_ev, s));
  mp->written = true;
  rc = mp->stage.back_and_wait(s, o_st, blk.size, "cms_mpstore_refresh");
  if (rc) return rc;
  std::memcpy(status, h + o_st, (size_t)n);
  for (int i = 0; i < n; ++i)
    if (status[i] == CMS_MP_DONE)
      mp->state[(size_t)ids[i]] |= ((what & CMS_MP_DESCRIPTOR) ? CMS_MP_ROW_DESC : 0) | ((what & CMS_MP_NORMAL_DEPTH) ? CMS_MP_ROW_NORMAL : 0);
  return CMS_OK;
}

// k_mp_gather of n ids (device) into the given device places, on stream s
static int mpstore_gather(const cms_mpstore* mp, hipStream_t s, int n, const int* d_ids, float* pos, float* normal, float* min_dist, float* max_dist, uint8_t* desc,
                          int* best_member, int* best_feature) {
  CmsMpGather g;
  g.t = mp->t; g.n = n; g.ids = d_ids; g.pos = pos; g.normal = normal; g.min_dist = min_dist; g.max_dist = max_dist; g.desc = (uint4*)desc;
  g.best_member = best_member; g.best_feature = best_feature;
  hipLaunchKernelGGL(k_mp_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g);
  HIPCHK(hipGetLastError());
  return CMS_OK;
}

extern "C" int cms_mpstore_fetch(cms_mpstore* mp, int n, const int* ids, float* pos, float* normal, float* min_dist, float* max_dist, uint8_t* desc,
                                 int* best_member, int* best_feature) {
  if (!mp || n < 0 || (n > 0 && !ids)) return cms_fail(CMS_ERR_ARG, "cms_mpstore_fetch: bad argument");
  if (n == 0) return CMS_OK;
  std::lock_guard<std::mutex> lk(mp->mu);
  if (const char* why = mpstore_check_ids(mp, n, ids, false)) return mpstore_fail("cms_mpstore_fetch", why);
  cms_ctx* c = mp->st->c;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t n4 = 4 * (size_t)n;
  CmsBlock blk;
  const size_t o_ids = blk.take(n4), in_bytes = blk.size, o_pos = blk.take(3 * n4), o_nrm = blk.take(3 * n4), o_min = blk.take(n4), o_max = blk.take(n4),
               o_desc = blk.take(32 * (size_t)n), o_bm = blk.take(n4), o_bf = blk.take(n4);
  int rc = mp->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = mp->stage.h;
  uint8_t* d = mp->stage.d;
  std::memcpy(h + o_ids, ids, n4);
  rc = mp->stage.up(s, in_bytes, "cms_mpstore_fetch");
  if (rc) return rc;
  rc = mpstore_gather(mp, s, n, (const int*)(d + o_ids), (float*)(d + o_pos), (float*)(d + o_nrm), (float*)(d + o_min), (float*)(d + o_max), d + o_desc, (int*)(d + o_bm),
                      (int*)(d + o_bf));
  if (rc) return rc;
  rc = mp->stage.back_and_wait(s, o_pos, blk.size, "cms_mpstore_fetch");
  if (rc) return rc;
  if (pos) std::memcpy(pos, h + o_pos, 3 * n4);
  if (normal) std::memcpy(normal, h + o_nrm, 3 * n4);
  if (min_dist) std::memcpy(min_dist, h + o_min, n4);
  if (max_dist) std::memcpy(max_dist, h + o_max, n4);
  if (desc) std::memcpy(desc, h + o_desc, 32 * (size_t)n);
  if (best_member) std::memcpy(best_member, h + o_bm, n4);
  if (best_feature) std::memcpy(best_feature, h + o_bf, n4);
  return CMS_OK;
}

// ---- the two consumers.  Each checks the rows on the host, then hands its host-array sibling's launch chain a hook that uploads the ids and gathers
// pos / normal / min / max / desc into the staged block's places.  Table values are the raw mfMinDistance / mfMaxDistance: the context's
// cms_set_distance_bounds_mode is switched to 0 for the call.
static const char* mpstore_check_consumable(cms_mpstore* mp, int n, const int* ids) {
  if (const char* why = mpstore_check_ids(mp, n, ids, false)) return why;
  const uint8_t need = CMS_MP_ROW_SET | CMS_MP_ROW_DESC | CMS_MP_ROW_NORMAL;
  for (int i = 0; i < n; ++i) if ((mp->state[(size_t)ids[i]] & need) != need) return "a row without descriptor or normal (erased, or never refreshed)";
  return nullptr;
}
struct CmsRawBounds {      // the raw-bounds mode for the lifetime of the object
  cms_ctx* c; int was;
  explicit CmsRawBounds(cms_ctx* ctx) : c(ctx), was(ctx->dist_bounds_scaled) { c->dist_bounds_scaled = 0; }
  ~CmsRawBounds() { c->dist_bounds_scaled = was; }
};
// the ids through the table's own staging block onto stream s, the gather behind them
static CmsPointGather mpstore_gather_hook(cms_mpstore* mp, int n, const int* ids, const char* who) {
  return [mp, n, ids, who](hipStream_t s, float* pos, float* normal, float* min_dist, float* max_dist, uint8_t* desc) -> int {
    int rc = mp->stage.reserve(s, 4 * (size_t)n, 4 * (size_t)n);
    if (rc) return rc;
    std::memcpy(mp->stage.h, ids, 4 * (size_t)n);
    rc = mp->stage.up(s, 4 * (size_t)n, who);
    if (rc) return rc;
    return mpstore_gather(mp, s, n, (const int*)mp->stage.d, pos, normal, min_dist, max_dist, desc, nullptr, nullptr);
  };
}

extern "C" int cms_search_local_points_ids(cms_ctx* ctx, int b, const float* pose15, cms_mpstore* mp, int nmp, const int* ids, float viewing_cos_limit, float th,
                                           float nnratio, int th_high, int nkp, int* kp_mp, uint8_t* in_view, float* proj_x, float* proj_y, int* level,
                                           float* view_cos, int* mp_match, int* n_matches, int* rounds) {
  if (!ctx || !mp || nmp < 0 || (nmp > 0 && !ids)) return cms_fail(CMS_ERR_ARG, "cms_search_local_points_ids: bad argument");
  if (ctx->device != mp->st->c->device) return cms_fail(CMS_ERR_ARG, "cms_search_local_points_ids: the frame context and the store must share the device");
  std::lock_guard<std::mutex> lk(mp->mu);
  if (const char* why = mpstore_check_consumable(mp, nmp, ids)) return mpstore_fail("cms_search_local_points_ids", why);
  HIPCHK(hipSetDevice(ctx->device));
  if (mp->written) HIPCHK(hipStreamWaitEvent(ctx->stream, mp->write_ev, 0));      // the table's last write ran on the store's stream
  const CmsRawBounds raw(ctx);
  const CmsPointGather gather = mpstore_gather_hook(mp, nmp, ids, "cms_search_local_points_ids");
  return track_search_local_one_frame(ctx, "cms_search_local_points_ids", b, pose15, nmp, nullptr, nullptr, nullptr, nullptr, nullptr, &gather, viewing_cos_limit, th, nnratio, th_high, nkp, kp_mp,
                                      in_view, proj_x, proj_y, level, view_cos, mp_match, n_matches, rounds);
}

extern "C" int cms_kfstore_fuse_search_sets_ids(cms_kfstore* st, cms_mpstore* mp, int nsets, const int* set_off, const int* ids, int njobs, const int* job_slot,
                                                const int* job_set, const uint8_t* skip, float th, int* best_idx, int* best_dist) {
  if (!st || !mp || nsets < 0 || (nsets > 0 && !set_off)) return cms_fail(CMS_ERR_ARG, "cms_kfstore_fuse_search_sets_ids: bad argument");
  if (mp->st != st) return cms_fail(CMS_ERR_ARG, "cms_kfstore_fuse_search_sets_ids: the table belongs to another store");
  const int npts = nsets > 0 ? set_off[nsets] : 0;
  if (npts < 0 || (npts > 0 && !ids)) return cms_fail(CMS_ERR_ARG, "cms_kfstore_fuse_search_sets_ids: bad argument");
  std::lock_guard<std::mutex> lk(mp->mu);
  if (const char* why = mpstore_check_consumable(mp, npts, ids)) return mpstore_fail("cms_kfstore_fuse_search_sets_ids", why);
  const CmsRawBounds raw(st->c);
  const CmsPointGather gather = mpstore_gather_hook(mp, npts, ids, "cms_kfstore_fuse_search_sets_ids");
  return kfstore_fuse_sets(st, nsets, set_off, nullptr, nullptr, nullptr, nullptr, nullptr, &gather, njobs, job_slot, job_set, skip, th, best_idx, best_dist);
}
