// cms_api_area.hip -- host side of the frame grid + window query (Frame::AssignFeaturesToGrid / GetFeaturesInArea), included by
// cms_lib.hip after cms_api_frames.hip (uses cms_ctx, cms_fail, HIPCHK, the context's CmsStage and the helpers of cms_api_util.h).  cms_area_args /
// cms_area_queries / cms_area_launch are the only place that fills and launches the window query's two kernels: the frame entries below and
// the key-frame store's Fuse (cms_api_tri.hip) go through them.
#include <vector>

// the rank sort of k_area_grid keeps 8 bytes per key point in LDS: above the 64 KB default for the 3 x nFeatures extractor of the
// initialisation.  Every launcher of the kernel (frame grids, key-frame store) calls this.
static int cms_area_grid_attr(int device) {
  static bool done[64] = {false};
  return cms_lds_ceiling_once((const void*)k_area_grid, (CMS_AREA_MAXKP + 1) * 8, device, done);
}
static int cms_area_reserve(cms_ctx* c) {
  if (c->d_area_sorted) return CMS_OK;
  if (c->g.kp_cap > CMS_AREA_MAXKP) return cms_fail(CMS_ERR_UNSUPPORTED, "frame grid: more than 16383 key points per frame");
  { const int rca = cms_area_grid_attr(c->device); if (rca) return rca; }
  const size_t B = (size_t)c->max_batch;
  HIPCHK(hipMalloc((void**)&c->d_area_sorted, B * c->g.kp_cap * sizeof(uint16_t)));
  HIPCHK(hipMalloc((void**)&c->d_area_cell_start, B * (CMS_AREA_CELLS + 1) * sizeof(int)));
  HIPCHK(hipMalloc((void**)&c->d_area_nvalid, B * sizeof(int)));
  return CMS_OK;
}

// per-context buffers of the window query: the first hits of every query (CMS_AREA_TMP entries each) and one partial sum of counts per
// search workgroup.  Both are written in full by launch 1 before launch 2 reads them and belong to the context whose stream the call runs
// on (every caller passes c->stream), so calls on one context are ordered and nothing has to be cleared between them.
static int cms_area_tmp_reserve(cms_ctx* c, int nq) {
  if ((size_t)nq <= c->area_tmp_cap) return CMS_OK;
  if (c->d_area_tmp) hipFree(c->d_area_tmp);
  c->d_area_tmp = nullptr; c->area_tmp_cap = 0;
  const size_t cap = (size_t)nq + (size_t)nq / 4 + 1024;
  HIPCHK(hipMalloc((void**)&c->d_area_tmp, cap * CMS_AREA_TMP * sizeof(int)));
  c->area_tmp_cap = cap;
  return CMS_OK;
}
static int cms_area_psum_reserve(cms_ctx* c, int nparts) {
  if (nparts <= c->area_psum_cap) return CMS_OK;
  if (c->d_area_psum) hipFree(c->d_area_psum);
  c->d_area_psum = nullptr; c->area_psum_cap = 0;
  const int cap = nparts + nparts / 4 + 64;
  HIPCHK(hipMalloc((void**)&c->d_area_psum, (size_t)cap * sizeof(int)));
  c->area_psum_cap = cap;
  return CMS_OK;
}

// ---- the window query: ONE place fills the grid side of its arguments and ONE place launches it.
// cms_area_args: a zeroed CmsAreaArgs over a grid source -- the context's frame grids or a key-frame store's slot grids (kp_cap = the frame
// stride of kp / sorted_idx); cms_area_queries adds the caller's queries and outputs (device pointers).
static CmsAreaArgs cms_area_args(const CmsKeyPoint* kp, const uint16_t* sorted_idx, const int* cell_start, int kp_cap, int F, float inv) {
  CmsAreaArgs a = {};
  a.kp = kp; a.sorted_idx = sorted_idx; a.cell_start = cell_start; a.kp_cap = kp_cap; a.F = F; a.inv = inv;
  return a;
}
static CmsAreaArgs cms_area_args_frames(const cms_ctx* c, int b) {      // frame b of the context's batch (queries with a q_frame: b = 0)
  return cms_area_args((const CmsKeyPoint*)c->d_kps + (size_t)b * c->g.kp_cap, c->d_area_sorted + (size_t)b * c->g.kp_cap,
                       c->d_area_cell_start + (size_t)b * (CMS_AREA_CELLS + 1), c->g.kp_cap, c->g.F, cms_grid_inv(c));
}
static void cms_area_queries(CmsAreaArgs& a, int nq, const void* q_frame, const void* qx, const void* qy, const void* qr, const void* qmin, const void* qmax,
                             void* cnt, void* off, void* idx, int cap, int idx_base) {
  a.nq = nq; a.q_frame = (const int*)q_frame;
  a.qx = (const float*)qx; a.qy = (const float*)qy; a.qr = (const float*)qr; a.qmin = (const int*)qmin; a.qmax = (const int*)qmax;
  a.cnt = (int*)cnt; a.off = (int*)off; a.idx = (int*)idx; a.cap = cap; a.idx_base = idx_base;
}
// The per-entry staging columns of the Fuse-shaped entries (cms_fuse_search, kfstore_fuse_core, cms_kfstore_search_by_sim3, sim3p_core): what the
// projection kernel writes (window, predicted level, the slot or frame whose grid is searched, the map-point record) and the window query's
// counts and offsets (one entry more).  take() lays them out in the entry's block, at() gives the pointers once the block's address is known;
// the candidate lists start at `o_idx`, behind everything else the entry staged.
struct CmsWindowCols {
  size_t o0 = 0, stride = 0;
  float *qx, *qy, *qr; int *qmin, *qmax, *level, *slot, *rec, *cnt, *off, *idx;
  void take(CmsBlock& b, size_t E) {
    o0 = b.size; stride = cms_align(E * 4);
    for (int k = 0; k < 9; ++k) b.take(E * 4);
    b.take(E * 4, 4);
  }
  void at(uint8_t* p, size_t o_idx) {
    float* f = (float*)(p + o0); int* i = (int*)(p + o0);
    const size_t n = stride / 4;
    qx = f; qy = f + n; qr = f + 2 * n; qmin = i + 3 * n; qmax = i + 4 * n; level = i + 5 * n; slot = i + 6 * n; rec = i + 7 * n; cnt = i + 8 * n; off = i + 9 * n;
    idx = (int*)(p + o_idx);
  }
};
static void cms_area_queries(CmsAreaArgs& a, int nq, const CmsWindowCols& w, int cap) {
  cms_area_queries(a, nq, w.slot, w.qx, w.qy, w.qr, w.qmin, w.qmax, w.cnt, w.off, w.idx, cap, 0);
}
// Two launches, ordered by the stream: the search (counts, first CMS_AREA_TMP hits of every query, one sum of counts per workgroup), then
// offsets + *d_total + lists per tile of queries (copied first hits; only a query with more candidates than that is searched again).
static int cms_area_launch(cms_ctx* c, hipStream_t s, CmsAreaArgs a, void* d_total) {
  const int nq = a.nq, qgrid = cms_area_search_grid(nq);
  int rc = cms_area_psum_reserve(c, qgrid);
  if (rc) return rc;
  rc = cms_area_tmp_reserve(c, nq);
  if (rc) return rc;
  a.tmp = c->d_area_tmp; a.psum = c->d_area_psum;
  hipLaunchKernelGGL(k_area_query, dim3(qgrid), dim3(CMS_AREA_QT), 0, s, a);
  hipLaunchKernelGGL(k_area_lists, dim3(cms_area_tile_grid(nq)), dim3(CMS_AREA_LT), 0, s, a, (int*)d_total);      // (writes at most a.cap candidates; *d_total > cap tells the caller)
  HIPCHK(hipGetLastError());
  return CMS_OK;
}

extern "C" int cms_area_set_keypoints(cms_ctx* c, int b, int n, const cms_keypoint* kps) {
  if (!c || b < 0 || b >= c->max_batch || n < 0 || n > c->g.kp_cap || (n > 0 && !kps)) return cms_fail(CMS_ERR_ARG, "cms_area_set_keypoints: bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (n > 0) HIPCHK(hipMemcpyAsync(c->d_kps + (size_t)b * c->g.kp_cap, kps, (size_t)n * sizeof(cms_keypoint), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->d_kp_cnt + b, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return CMS_OK;
}

extern "C" int cms_area_grid(cms_ctx* c, int B) {
  if (!c || B < 1 || B > c->max_batch) return cms_fail(CMS_ERR_ARG, "cms_area_grid: bad batch");
  HIPCHK(hipSetDevice(c->device));
  int rc = cms_area_reserve(c);
  if (rc) return rc;
  hipLaunchKernelGGL(k_area_grid, dim3(B), dim3(1024), (size_t)(c->g.kp_cap + 1) * 8, c->stream, (const CmsKeyPoint*)c->d_kps, (const int*)c->d_kp_cnt, c->g.kp_cap, c->g.F, cms_grid_inv(c),
                     c->d_area_sorted, c->d_area_cell_start, c->d_area_nvalid);
  HIPCHK(hipGetLastError());
  c->area_frames = B;
  return CMS_OK;
}

extern "C" int cms_features_in_area_device(cms_ctx* c, int b, int nq, const void* d_qx, const void* d_qy, const void* d_qr, const void* d_qmin,
                                           const void* d_qmax, void* d_cnt_scratch, void* d_cand_off, void* d_cand_idx, int cap, int idx_base,
                                           void* d_total) {
  if (!c || b < 0 || b >= c->area_frames || nq < 0 || cap < 0) return cms_fail(CMS_ERR_ARG, "cms_features_in_area_device: bad argument (cms_area_grid first)");
  if (nq == 0) return CMS_OK;
  HIPCHK(hipSetDevice(c->device));
  CmsAreaArgs a = cms_area_args_frames(c, b);
  cms_area_queries(a, nq, nullptr, d_qx, d_qy, d_qr, d_qmin, d_qmax, d_cnt_scratch, d_cand_off, d_cand_idx, cap, idx_base);
  return cms_area_launch(c, c->stream, a, d_total);
}

// every query names the frame of the batch it searches (d_qframe); candidate indices are rows of the batch (frame * kp_cap + i)
extern "C" int cms_features_in_area_batch_device(cms_ctx* c, int nq, const void* d_qframe, const void* d_qx, const void* d_qy, const void* d_qr,
                                                 const void* d_qmin, const void* d_qmax, void* d_cnt_scratch, void* d_cand_off, void* d_cand_idx,
                                                 int cap, void* d_total) {
  if (!c || nq < 0 || cap < 0 || c->area_frames < 1 || !d_qframe) return cms_fail(CMS_ERR_ARG, "cms_features_in_area_batch_device: bad argument (cms_area_grid first)");
  if (nq == 0) return CMS_OK;
  HIPCHK(hipSetDevice(c->device));
  CmsAreaArgs a = cms_area_args_frames(c, 0);
  cms_area_queries(a, nq, d_qframe, d_qx, d_qy, d_qr, d_qmin, d_qmax, d_cnt_scratch, d_cand_off, d_cand_idx, cap, 0);
  return cms_area_launch(c, c->stream, a, d_total);
}

extern "C" int cms_features_in_area(cms_ctx* c, int b, int nq, const float* qx, const float* qy, const float* qr, const int* qmin, const int* qmax,
                                    int* cand_off, int* cand_idx, int cap, int* total) {
  if (!c || nq < 0 || cap < 0 || !cand_off || (nq > 0 && (!qx || !qy || !qr || !qmin || !qmax))) return cms_fail(CMS_ERR_ARG, "cms_features_in_area: bad argument");
  if (b < 0 || b >= c->area_frames) return cms_fail(CMS_ERR_ARG, "cms_features_in_area: no grid for this frame (cms_area_grid first)");
  cand_off[0] = 0;
  if (total) *total = 0;
  if (nq == 0) return CMS_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t qb = (size_t)nq * 4;
  const size_t bytes = 5 * qb + qb /*cnt*/ + (qb + 4) /*off*/ + (size_t)cap * 4 + 64;
  hipStream_t s = c->stream;
  int rc = c->stage.reserve(s, bytes, 0);
  if (rc) return rc;
  uint8_t* p = c->stage.d;
  void* dq[5];
  const void* hq[5] = {qx, qy, qr, qmin, qmax};
  for (int i = 0; i < 5; ++i) { dq[i] = p; p += qb; HIPCHK(hipMemcpyAsync(dq[i], hq[i], qb, hipMemcpyHostToDevice, s)); }
  void* d_cnt = p; p += qb;
  void* d_off = p; p += qb + 4;
  void* d_tot = p; p += 16;
  void* d_idx = p;
  rc = cms_features_in_area_device(c, b, nq, dq[0], dq[1], dq[2], dq[3], dq[4], d_cnt, d_off, d_idx, cap, 0, d_tot);
  if (rc) return rc;
  int tot = 0;
  HIPCHK(hipMemcpyAsync(cand_off, d_off, qb + 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&tot, d_tot, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (total) *total = tot;
  if (tot > cap) return cms_fail(CMS_ERR_OVERFLOW, "cms_features_in_area: candidate capacity too small");
  if (tot > 0 && cand_idx) HIPCHK(hipMemcpy(cand_idx, d_idx, (size_t)tot * 4, hipMemcpyDeviceToHost));
  return CMS_OK;
}
