// cms_api_covis.hip -- host side of the covisibility entries (cms_covis_*) and of cms_kfstore_update_map_points.  Included by cms_lib.hip behind
// cms_api_tri.hip (cms_kfstore) and cms_covis_kernels.hip.  A cms_covis is an observation index over member slots of ONE store: cms_covis_build
// snapshots the members' mp rows and octaves on the store's stream and builds the table there; a query runs on the stream its entry names, waits
// ON THE DEVICE for the last build (an event) and answers from it: one upload, one launch, one copy back, one wait (CmsStage).  Calls on one handle
// are serialised by its mutex; queries are synchronous, so nothing of the handle is in flight when the next call starts.
#include <cstring>
#include <initializer_list>
#include <vector>

struct cms_covis {
  std::mutex mu;
  cms_kfstore* st = nullptr;
  int max_members = 0;
  bool built = false;
  int M = 0, bits = 8;
  size_t sum_n = 0;                         // the members' features: the bound of observations and of ids
  std::vector<int> h_n;                     // features per member at the last build (cms_covis_local_ba_windows sizes its point lists by them)
  // capacities: members, table entries, observations
  size_t cap_m = 0, cap_rows = 0, cap_h = 0, cap_o = 0, cap_of = 0, cap_dec = 0;
  int* d_slot = nullptr; int* d_n = nullptr; int* d_snap_u = nullptr; int* d_snap_oct = nullptr;
  int* d_key = nullptr; int* d_cnt = nullptr; int* d_off = nullptr; int* d_uix = nullptr; int* d_cur = nullptr; int2* d_obs = nullptr; int* d_obs_feat = nullptr;
  int* d_counters = nullptr; int* d_dec = nullptr;
  hipEvent_t built_ev = nullptr;
  CmsStage stage;
};

static void covis_free(void* p) { if (p) (void)hipFree(p); }
extern "C" void cms_covis_destroy(cms_covis* cv) {
  if (!cv) return;
  if (cv->st && cv->st->c) (void)hipSetDevice(cv->st->c->device);
  void* bufs[] = {cv->d_slot, cv->d_n, cv->d_snap_u, cv->d_snap_oct, cv->d_key, cv->d_cnt, cv->d_off, cv->d_uix, cv->d_cur, cv->d_obs, cv->d_obs_feat, cv->d_counters, cv->d_dec};
  for (void* b : bufs) covis_free(b);
  if (cv->built_ev) (void)hipEventDestroy(cv->built_ev);
  cv->stage.release();
  delete cv;
}
extern "C" int cms_covis_create(cms_covis** out, cms_kfstore* st, int max_members) {
  if (!out || !st || max_members < 1) return cms_fail(CMS_ERR_ARG, "cms_covis_create: bad argument");
  if (max_members > CMS_COVIS_MAX_MEMBERS) return cms_fail(CMS_ERR_UNSUPPORTED, "cms_covis_create: at most 16384 members");
  HIPCHK(hipSetDevice(st->c->device));
  cms_covis* cv = new cms_covis();
  cv->st = st; cv->max_members = max_members;
  if (hipEventCreateWithFlags(&cv->built_ev, hipEventDisableTiming) != hipSuccess || hipMalloc((void**)&cv->d_counters, 8) != hipSuccess) {
    cms_covis_destroy(cv);
    return cms_fail(CMS_ERR_HIP, "cms_covis_create: out of device memory");
  }
  *out = cv;
  return CMS_OK;
}

// n elements in each of the listed buffers (the streams that used the old blocks are idle: see the head of the file); `have` is their common capacity
static int covis_grow(std::initializer_list<void**> bufs, size_t& have, size_t need, size_t elem) {
  if (need <= have) return CMS_OK;
  have = 0;
  for (void** p : bufs) if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; }
  const size_t want = need + need / 4 + 64;
  for (void** p : bufs) HIPCHK(hipMalloc(p, want * elem));
  have = want;
  return CMS_OK;
}
static CmsCovisDev covis_dev(const cms_covis* cv) {
  CmsCovisDev d;
  d.M = cv->M; d.maxf = cv->st->maxf; d.bits = cv->bits; d.n = cv->d_n; d.snap_u = cv->d_snap_u; d.snap_oct = cv->d_snap_oct;
  d.key = cv->d_key; d.cnt = cv->d_cnt; d.off = cv->d_off; d.uix = cv->d_uix; d.obs = cv->d_obs; d.obs_feat = cv->d_obs_feat; d.slot = cv->d_slot;
  return d;
}

extern "C" int cms_covis_build(cms_covis* cv, int n_members, const int* member_slots) {
  if (!cv || n_members < 0 || (n_members > 0 && !member_slots)) return cms_fail(CMS_ERR_ARG, "cms_covis_build: bad argument");
  if (n_members > CMS_COVIS_MAX_MEMBERS) return cms_fail(CMS_ERR_UNSUPPORTED, "cms_covis_build: more than 16384 members");
  if (n_members > cv->max_members) return cms_fail(CMS_ERR_ARG, "cms_covis_build: more members than the handle was created for");
  std::lock_guard<std::mutex> lk(cv->mu);
  cms_kfstore* st = cv->st;
  const size_t M = (size_t)n_members;
  size_t sum_n = 0;
  int max_n = 0;
  {
    std::vector<uint8_t> seen((size_t)st->maxkf, 0);
    for (size_t m = 0; m < M; ++m) {
      const int s = member_slots[m];
      if (s < 0 || s >= st->maxkf || !st->used[(size_t)s]) return cms_fail(CMS_ERR_ARG, "cms_covis_build: a member slot is empty");
      if (seen[(size_t)s]) return cms_fail(CMS_ERR_ARG, "cms_covis_build: a slot is named twice");
      seen[(size_t)s] = 1;
      sum_n += (size_t)st->h_kf[(size_t)s].n; max_n = std::max(max_n, st->h_kf[(size_t)s].n);
    }
  }
  if (sum_n > ((size_t)1 << 28)) return cms_fail(CMS_ERR_UNSUPPORTED, "cms_covis_build: more than 2^28 features among the members");
  cms_ctx* c = st->c;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(kfstore_order_behind_puts(st));
  hipStream_t s = c->stream;
  if (M == 0) { cv->M = 0; cv->sum_n = 0; cv->h_n.clear(); cv->built = true; HIPCHK(hipEventRecord(cv->built_ev, s)); return CMS_OK; }
  // ---- the rows first: a row that names an id twice refuses the build before anything of the index is touched
  CmsBlock blk;
  const size_t o_slot = blk.take(4 * M), o_n = blk.take(4 * M), o_flag = blk.take(4), in_bytes = blk.size;
  int rc = cv->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = cv->stage.h;
  uint8_t* d = cv->stage.d;
  int* h_slot = reinterpret_cast<int*>(h + o_slot);
  int* h_n = reinterpret_cast<int*>(h + o_n);
  for (size_t m = 0; m < M; ++m) { h_slot[m] = member_slots[m]; h_n[m] = st->h_kf[(size_t)member_slots[m]].n; st->busy[(size_t)member_slots[m]] = 1; }
  *reinterpret_cast<int*>(h + o_flag) = 0;
  rc = cv->stage.up(s, in_bytes, "cms_covis_build");
  if (rc) return rc;
  int P = 2;
  while (P < max_n) P <<= 1;      // <= 16384 ints: inside the 64 KB a kernel may ask for without an attribute
  hipLaunchKernelGGL(k_covis_rowcheck, dim3((unsigned)M), dim3(256), 4 * (size_t)P, s, (const int*)(d + o_slot), (const int*)(d + o_n), (const int*)st->d_mp, st->maxf, P,
                     (int*)(d + o_flag));
  HIPCHK(hipGetLastError());
  rc = cv->stage.back_and_wait(s, o_flag, o_flag + 4, "cms_covis_build");
  if (rc) return rc;
  if (*reinterpret_cast<const int*>(h + o_flag)) return cms_fail(CMS_ERR_ARG, "cms_covis_build: a member's row names a map point twice (the previous index stays)");
  // ---- the index: from here the previous one is gone
  cv->built = false;
  int bits = 8;
  while (((size_t)1 << bits) < 2 * sum_n) ++bits;
  const size_t H = (size_t)1 << bits;
  if ((rc = covis_grow({(void**)&cv->d_slot, (void**)&cv->d_n}, cv->cap_m, M, 4))) return rc;
  if ((rc = covis_grow({(void**)&cv->d_snap_u, (void**)&cv->d_snap_oct}, cv->cap_rows, M * (size_t)st->maxf, 4))) return rc;
  if ((rc = covis_grow({(void**)&cv->d_key, (void**)&cv->d_cnt, (void**)&cv->d_off, (void**)&cv->d_uix, (void**)&cv->d_cur}, cv->cap_h, H, 4))) return rc;
  if ((rc = covis_grow({(void**)&cv->d_obs}, cv->cap_o, std::max(sum_n, (size_t)1), sizeof(int2)))) return rc;
  if ((rc = covis_grow({(void**)&cv->d_obs_feat}, cv->cap_of, std::max(sum_n, (size_t)1), 4))) return rc;
  HIPCHK(hipMemcpyAsync(cv->d_slot, d + o_slot, 4 * M, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(cv->d_n, d + o_n, 4 * M, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemsetAsync(cv->d_key, 0xFF, 4 * H, s));
  HIPCHK(hipMemsetAsync(cv->d_cnt, 0, 4 * H, s));
  HIPCHK(hipMemsetAsync(cv->d_cur, 0, 4 * H, s));
  HIPCHK(hipMemsetAsync(cv->d_counters, 0, 8, s));
  CmsCovisBuild a;
  a.M = n_members; a.maxf = st->maxf; a.bits = bits; a.st_maxf = st->maxf; a.slot = cv->d_slot; a.n = cv->d_n; a.st_mp = st->d_mp; a.st_kp = st->d_kp;
  a.snap_u = cv->d_snap_u; a.snap_oct = cv->d_snap_oct; a.key = cv->d_key; a.cnt = cv->d_cnt; a.off = cv->d_off; a.uix = cv->d_uix; a.cur = cv->d_cur; a.obs = cv->d_obs; a.obs_feat = cv->d_obs_feat;
  a.counters = cv->d_counters;
  if (max_n > 0) {
    const dim3 rows((unsigned)((max_n + 255) / 256), (unsigned)M);
    hipLaunchKernelGGL(k_covis_insert, rows, dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_covis_alloc, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_covis_fill, rows, dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(cv->built_ev, s));
  cv->M = n_members; cv->bits = bits; cv->sum_n = sum_n; cv->built = true;
  cv->h_n.assign(h_n, h_n + M);      // (the stage's pinned block still holds them: nothing has reserved it since)
  return CMS_OK;
}

static int covis_ready(const cms_covis* cv, const char* who) {
  if (!cv->built) return cms_fail(CMS_ERR_ARG, (std::string(who) + ": no index (cms_covis_build first)").c_str());
  return CMS_OK;
}
// the three kernels with the members' counters in LDS may ask for more than 64 KB
static int covis_lds(const void* kernel, int device, bool (&done)[64]) { return cms_lds_ceiling_once(kernel, CMS_COVIS_MAX_MEMBERS * 8, device, done); }

extern "C" int cms_covis_votes(cms_covis* cv, cms_ctx* src, int njobs, const int* id_off, const int* ids, int* votes) {
  if (!cv || !src || njobs < 0 || (njobs > 0 && !id_off)) return cms_fail(CMS_ERR_ARG, "cms_covis_votes: bad argument");
  if (njobs == 0) return CMS_OK;
  if (src->device != cv->st->c->device) return cms_fail(CMS_ERR_ARG, "cms_covis_votes: the frame context and the store must share the device");
  if (id_off[0] != 0) return cms_fail(CMS_ERR_ARG, "cms_covis_votes: id_off must start at 0");
  for (int j = 0; j < njobs; ++j) if (id_off[j + 1] < id_off[j]) return cms_fail(CMS_ERR_ARG, "cms_covis_votes: id_off must not descend");
  const size_t T = (size_t)id_off[njobs], Q = (size_t)njobs;
  if (T > 0 && !ids) return cms_fail(CMS_ERR_ARG, "cms_covis_votes: bad argument");
  for (size_t q = 0; q < T; ++q) if (ids[q] < 0) return cms_fail(CMS_ERR_ARG, "cms_covis_votes: a negative id");
  std::lock_guard<std::mutex> lk(cv->mu);
  int rc = covis_ready(cv, "cms_covis_votes");
  if (rc) return rc;
  const size_t M = (size_t)cv->M;
  if (M == 0) return CMS_OK;
  if (!votes) return cms_fail(CMS_ERR_ARG, "cms_covis_votes: bad argument");
  HIPCHK(hipSetDevice(src->device));
  hipStream_t s = src->stream;
  HIPCHK(hipStreamWaitEvent(s, cv->built_ev, 0));
  CmsBlock blk;
  const size_t o_off = blk.take(4 * (Q + 1)), o_ids = blk.take(4 * T), in_bytes = blk.size, o_votes = blk.take(4 * Q * M);
  rc = cv->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = cv->stage.h;
  uint8_t* d = cv->stage.d;
  std::memcpy(h + o_off, id_off, 4 * (Q + 1));
  if (T > 0) std::memcpy(h + o_ids, ids, 4 * T);
  rc = cv->stage.up(s, in_bytes, "cms_covis_votes");
  if (rc) return rc;
  static bool lds_done[64] = {};
  rc = covis_lds((const void*)k_covis_votes, src->device, lds_done);
  if (rc) return rc;
  hipLaunchKernelGGL(k_covis_votes, dim3((unsigned)njobs), dim3(1024), 4 * M, s, covis_dev(cv), (const int*)(d + o_off), (const int*)(d + o_ids), (int*)(d + o_votes));
  HIPCHK(hipGetLastError());
  rc = cv->stage.back_and_wait(s, o_votes, blk.size, "cms_covis_votes");
  if (rc) return rc;
  std::memcpy(votes, h + o_votes, 4 * Q * M);
  return CMS_OK;
}

extern "C" int cms_covis_connections(cms_covis* cv, int njobs, const int* job_member, int th, int* weights, int* order, int* n_connected) {
  if (!cv || njobs < 0 || (njobs > 0 && (!job_member || !weights || !order || !n_connected))) return cms_fail(CMS_ERR_ARG, "cms_covis_connections: bad argument");
  if (njobs == 0) return CMS_OK;
  std::lock_guard<std::mutex> lk(cv->mu);
  int rc = covis_ready(cv, "cms_covis_connections");
  if (rc) return rc;
  for (int j = 0; j < njobs; ++j) if (job_member[j] < 0 || job_member[j] >= cv->M) return cms_fail(CMS_ERR_ARG, "cms_covis_connections: a job names no member");
  const size_t M = (size_t)cv->M, Q = (size_t)njobs;
  cms_ctx* c = cv->st->c;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  CmsBlock blk;
  const size_t o_job = blk.take(4 * Q), in_bytes = blk.size, o_w = blk.take(4 * Q * M), o_ord = blk.take(4 * Q * M), o_nc = blk.take(4 * Q);
  rc = cv->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = cv->stage.h;
  uint8_t* d = cv->stage.d;
  std::memcpy(h + o_job, job_member, 4 * Q);
  rc = cv->stage.up(s, in_bytes, "cms_covis_connections");
  if (rc) return rc;
  static bool lds_done[64] = {};
  rc = covis_lds((const void*)k_covis_connections, c->device, lds_done);
  if (rc) return rc;
  hipLaunchKernelGGL(k_covis_connections, dim3((unsigned)njobs), dim3(1024), 8 * M, s, covis_dev(cv), (const int*)(d + o_job), th, (int*)(d + o_w), (int*)(d + o_ord), (int*)(d + o_nc));
  HIPCHK(hipGetLastError());
  rc = cv->stage.back_and_wait(s, o_w, blk.size, "cms_covis_connections");
  if (rc) return rc;
  std::memcpy(weights, h + o_w, 4 * Q * M); std::memcpy(order, h + o_ord, 4 * Q * M); std::memcpy(n_connected, h + o_nc, 4 * Q);
  return CMS_OK;
}

extern "C" int cms_covis_culling(cms_covis* cv, int n_chains, const int* chain_off, const int* job_member, const uint8_t* erasable, int th_obs, int* n_mps,
                                 int* n_redundant, uint8_t* redundant) {
  if (!cv || n_chains < 0 || th_obs < 0 || (n_chains > 0 && !chain_off)) return cms_fail(CMS_ERR_ARG, "cms_covis_culling: bad argument");
  if (n_chains == 0) return CMS_OK;
  if (chain_off[0] != 0) return cms_fail(CMS_ERR_ARG, "cms_covis_culling: chain_off must start at 0");
  for (int c = 0; c < n_chains; ++c) if (chain_off[c + 1] < chain_off[c]) return cms_fail(CMS_ERR_ARG, "cms_covis_culling: chain_off must not descend");
  const size_t Q = (size_t)chain_off[n_chains], C = (size_t)n_chains;
  if (Q == 0) return CMS_OK;
  if (!job_member || !erasable || !n_mps || !n_redundant || !redundant) return cms_fail(CMS_ERR_ARG, "cms_covis_culling: bad argument");
  std::lock_guard<std::mutex> lk(cv->mu);
  int rc = covis_ready(cv, "cms_covis_culling");
  if (rc) return rc;
  {
    std::vector<int> seen((size_t)cv->M, -1);
    for (int c = 0; c < n_chains; ++c)
      for (int j = chain_off[c]; j < chain_off[c + 1]; ++j) {
        if (job_member[j] < 0 || job_member[j] >= cv->M) return cms_fail(CMS_ERR_ARG, "cms_covis_culling: a job names no member");
        if (seen[(size_t)job_member[j]] == c) return cms_fail(CMS_ERR_ARG, "cms_covis_culling: a chain names a member twice");
        seen[(size_t)job_member[j]] = c;
      }
  }
  cms_ctx* ctx = cv->st->c;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t stride = std::max(cv->sum_n, (size_t)1);      // ids <= observations <= features
  // the scratch: one int per (chain, id), n_chains x the members' features at most (8 MB per chain for 1 000 x 2 000).  It is cleared when it is
  // (re)allocated; k_covis_culling zeroes what it touched before it ends, so a call costs no clearing pass
  {
    const size_t had = cv->cap_dec;
    if ((rc = covis_grow({(void**)&cv->d_dec}, cv->cap_dec, C * stride, 4))) return rc;
    if (cv->cap_dec != had) HIPCHK(hipMemsetAsync(cv->d_dec, 0, 4 * cv->cap_dec, s));
  }
  CmsBlock blk;
  const size_t o_off = blk.take(4 * (C + 1)), o_job = blk.take(4 * Q), o_er = blk.take(Q), in_bytes = blk.size;
  const size_t o_nm = blk.take(4 * Q), o_nr = blk.take(4 * Q), o_red = blk.take(Q);
  rc = cv->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = cv->stage.h;
  uint8_t* d = cv->stage.d;
  std::memcpy(h + o_off, chain_off, 4 * (C + 1)); std::memcpy(h + o_job, job_member, 4 * Q); std::memcpy(h + o_er, erasable, Q);
  rc = cv->stage.up(s, in_bytes, "cms_covis_culling");
  if (rc) return rc;
  hipLaunchKernelGGL(k_covis_culling, dim3((unsigned)n_chains), dim3(1024), 0, s, covis_dev(cv), (const int*)(d + o_off), (const int*)(d + o_job), (const uint8_t*)(d + o_er), th_obs,
                     cv->d_dec, stride, (int*)(d + o_nm), (int*)(d + o_nr), (uint8_t*)(d + o_red));
  HIPCHK(hipGetLastError());
  rc = cv->stage.back_and_wait(s, o_nm, blk.size, "cms_covis_culling");
  if (rc) return rc;
  std::memcpy(n_mps, h + o_nm, 4 * Q); std::memcpy(n_redundant, h + o_nr, 4 * Q); std::memcpy(redundant, h + o_red, Q);
  return CMS_OK;
}

extern "C" int cms_covis_local_points(cms_covis* cv, cms_ctx* src, int njobs, const int* kf_off, const int* kf_members, int cap, int* ids_out, int* n_out) {
  if (!cv || !src || njobs < 0 || cap < 0 || (njobs > 0 && (!kf_off || !n_out || (cap > 0 && !ids_out)))) return cms_fail(CMS_ERR_ARG, "cms_covis_local_points: bad argument");
  if (njobs == 0) return CMS_OK;
  if (src->device != cv->st->c->device) return cms_fail(CMS_ERR_ARG, "cms_covis_local_points: the frame context and the store must share the device");
  if (kf_off[0] != 0) return cms_fail(CMS_ERR_ARG, "cms_covis_local_points: kf_off must start at 0");
  for (int j = 0; j < njobs; ++j) if (kf_off[j + 1] < kf_off[j]) return cms_fail(CMS_ERR_ARG, "cms_covis_local_points: kf_off must not descend");
  const size_t T = (size_t)kf_off[njobs], Q = (size_t)njobs;
  if (T > 0 && !kf_members) return cms_fail(CMS_ERR_ARG, "cms_covis_local_points: bad argument");
  std::lock_guard<std::mutex> lk(cv->mu);
  int rc = covis_ready(cv, "cms_covis_local_points");
  if (rc) return rc;
  {
    std::vector<int> seen((size_t)cv->M, -1);
    for (int j = 0; j < njobs; ++j)
      for (int q = kf_off[j]; q < kf_off[j + 1]; ++q) {
        if (kf_members[q] < 0 || kf_members[q] >= cv->M) return cms_fail(CMS_ERR_ARG, "cms_covis_local_points: a job names no member");
        if (seen[(size_t)kf_members[q]] == j) return cms_fail(CMS_ERR_ARG, "cms_covis_local_points: a job names a member twice");
        seen[(size_t)kf_members[q]] = j;
      }
  }
  std::fill(n_out, n_out + Q, 0);
  if (T == 0) return CMS_OK;
  HIPCHK(hipSetDevice(src->device));
  hipStream_t s = src->stream;
  HIPCHK(hipStreamWaitEvent(s, cv->built_ev, 0));
  CmsBlock blk;
  const size_t o_off = blk.take(4 * (Q + 1)), o_kf = blk.take(4 * T), in_bytes = blk.size, o_n = blk.take(4 * Q), o_ids = blk.take(4 * Q * (size_t)cap);
  rc = cv->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = cv->stage.h;
  uint8_t* d = cv->stage.d;
  std::memcpy(h + o_off, kf_off, 4 * (Q + 1)); std::memcpy(h + o_kf, kf_members, 4 * T);
  rc = cv->stage.up(s, in_bytes, "cms_covis_local_points");
  if (rc) return rc;
  static bool lds_done[64] = {};
  rc = covis_lds((const void*)k_covis_local_points, src->device, lds_done);
  if (rc) return rc;
  hipLaunchKernelGGL(k_covis_local_points, dim3((unsigned)njobs), dim3(1024), 4 * (size_t)cv->M, s, covis_dev(cv), (const int*)(d + o_off), (const int*)(d + o_kf), cap, (int*)(d + o_ids),
                     (int*)(d + o_n));
  HIPCHK(hipGetLastError());
  rc = cv->stage.back_and_wait(s, o_n, blk.size, "cms_covis_local_points");
  if (rc) return rc;
  const int* hn = reinterpret_cast<const int*>(h + o_n);
  const int* hid = reinterpret_cast<const int*>(h + o_ids);
  bool overflow = false;
  for (size_t j = 0; j < Q; ++j) {
    n_out[j] = hn[j];
    overflow = overflow || hn[j] > cap;
    const size_t k = (size_t)std::min(hn[j], cap);
    if (k > 0) std::memcpy(ids_out + j * (size_t)cap, hid + j * (size_t)cap, 4 * k);
  }
  if (overflow) return cms_fail(CMS_ERR_OVERFLOW, "cms_covis_local_points: a job has more ids than cap (n_out says how many)");
  return CMS_OK;
}

// ---- Fuse's Replace and MapPointCulling change a handful of mp entries in many key frames: one kernel scatters (slot, feature, id) triples it reads
// from a pinned ring of four blocks, asynchronous on the store's stream like cms_kfstore_update_poses
struct CmsStoreMpUpd {
  int* h[4] = {nullptr, nullptr, nullptr, nullptr}; size_t cap[4] = {0, 0, 0, 0};
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; bool ev_set[4] = {false, false, false, false};
  unsigned call = 0;
};
static void cms_store_mpupd_free(CmsStoreMpUpd* u) {
  if (!u) return;
  for (int i = 0; i < 4; ++i) { if (u->h[i]) (void)hipHostFree(u->h[i]); if (u->ev[i]) (void)hipEventDestroy(u->ev[i]); }
  delete u;
}
extern "C" int cms_kfstore_update_map_points(cms_kfstore* st, int n, const int* slot, const int* feat, const int* mp) {
  if (!st || n < 0 || (n > 0 && (!slot || !feat || !mp))) return cms_fail(CMS_ERR_ARG, "cms_kfstore_update_map_points: bad argument");
  if (n == 0) return CMS_OK;
  {
    std::vector<unsigned long long> key((size_t)n);
    for (int i = 0; i < n; ++i) {
      if (slot[i] < 0 || slot[i] >= st->maxkf || !st->used[(size_t)slot[i]]) return cms_fail(CMS_ERR_ARG, "cms_kfstore_update_map_points: bad slot");
      if (feat[i] < 0 || feat[i] >= st->h_kf[(size_t)slot[i]].n) return cms_fail(CMS_ERR_ARG, "cms_kfstore_update_map_points: a feature index beyond the key frame");
      if (mp[i] < -1 || mp[i] > CMS_COVIS_MAX_ID) return cms_fail(CMS_ERR_ARG, "cms_kfstore_update_map_points: an id outside [-1, 2^30)");
      key[(size_t)i] = ((unsigned long long)(unsigned)slot[i] << 32) | (unsigned)feat[i];
    }
    std::sort(key.begin(), key.end());
    for (size_t i = 1; i < key.size(); ++i) if (key[i] == key[i - 1]) return cms_fail(CMS_ERR_ARG, "cms_kfstore_update_map_points: a (slot, feature) is named twice");
  }
  cms_ctx* c = st->c;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(kfstore_order_behind_puts(st));
  if (!st->mpupd) st->mpupd = new CmsStoreMpUpd();
  CmsStoreMpUpd* u = st->mpupd;
  const unsigned ring = u->call++ & 3;
  if (!u->ev[ring]) HIPCHK(hipEventCreateWithFlags(&u->ev[ring], hipEventDisableTiming));
  if (u->ev_set[ring]) HIPCHK(hipEventSynchronize(u->ev[ring]));      // the kernel that last read this block: four calls ago, long through
  if (u->cap[ring] < (size_t)n) {
    if (u->h[ring]) { HIPCHK(hipHostFree(u->h[ring])); u->h[ring] = nullptr; u->cap[ring] = 0; }
    const size_t want = (size_t)n + (size_t)n / 2 + 256;
    HIPCHK(hipHostMalloc((void**)&u->h[ring], want * 12, hipHostMallocMapped | hipHostMallocCoherent));
    u->cap[ring] = want;
  }
  int* t = u->h[ring];
  for (int i = 0; i < n; ++i) { t[3 * i] = slot[i]; t[3 * i + 1] = feat[i]; t[3 * i + 2] = mp[i]; st->busy[(size_t)slot[i]] = 1; }
  hipLaunchKernelGGL(k_kf_update_map_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, st->d_mp, st->maxf, (const int*)t, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(u->ev[ring], c->stream));
  u->ev_set[ring] = true;
  return CMS_OK;
}
