// cms_api_vocab.hip -- host side of Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cpp:719-726, src/KeyFrame.cpp:94-103): the cms_vocab handle
// and the entries that run ORBVocabulary::transform on the device.  Included by cms_lib.hip behind cms_api_bow.hip (cms_ctx and its CmsStage, cms_kfstore, bow_run)
// and cms_vocab_kernels.hip.  A call is ONE launch of k_vocab_descend over all features of all its rows and ONE launch of k_vocab_build (a
// workgroup per row); everything that becomes a device index (rows, slots, counts) is checked on the host before anything is enqueued.  The calls
// end with the rows' three counts on the host (words, nodes, listed features): the next step of the caller -- SearchByBoW, the key-frame database,
// CreateNewMapPoints -- needs them to size its own work.
#include <cstring>
#include <vector>

struct cms_vocab {
  int device = 0, group = 16;
  CmsVocabView dv = {};      // device pointers
  void* bufs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

extern "C" void cms_vocab_destroy(cms_vocab* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  for (void* b : v->bufs) if (b) (void)hipFree(b);
  delete v;
}

extern "C" int cms_vocab_create(cms_vocab** out, int device, int k, int L, int scoring, int weighting, int n_nodes, const int* parent, const uint8_t* is_leaf,
                                const uint8_t* desc, const double* weight) {
  if (!out) return cms_fail(CMS_ERR_ARG, "cms_vocab_create: bad argument");
  CmsVocabTree t;
  const char* why = cms_vocab_relayout(k, L, scoring, weighting, n_nodes, parent, is_leaf, desc, weight, &t);
  if (why) return cms_fail(CMS_ERR_ARG, (std::string("cms_vocab_create: ") + why).c_str());
  const int rcd = cms_check_device(device, "cms_vocab_create: no HIP device (the vocabulary's device path has no CPU fallback)");
  if (rcd) return rcd;
  HIPCHK(hipSetDevice(device));
  cms_vocab* v = new cms_vocab();
  v->device = device; v->group = k <= 16 ? 16 : 32;
  const size_t N = (size_t)t.n_nodes, W = (size_t)t.n_words;
  const void* src[5] = {t.info.data(), t.desc.data(), t.file_id.data(), t.word.data(), t.word_weight.data()};
  const size_t bytes[5] = {4 * N, 32 * N, 4 * N, 4 * N, 8 * W};
  for (int i = 0; i < 5; ++i) {
    hipError_t e = hipMalloc(&v->bufs[i], bytes[i]);
    if (e == hipSuccess) e = hipMemcpy(v->bufs[i], src[i], bytes[i], hipMemcpyHostToDevice);
    if (e != hipSuccess) { cms_vocab_destroy(v); return cms_fail(CMS_ERR_HIP, "cms_vocab_create: upload", e); }
  }
  v->dv = CmsVocabView{t.k, t.L, t.scoring, t.weighting, t.n_nodes, t.n_words, (const uint32_t*)v->bufs[0], (const uint32_t*)v->bufs[1], (const int*)v->bufs[2],
                       (const int*)v->bufs[3], (const double*)v->bufs[4]};
  *out = v;
  return CMS_OK;
}

// info[7]: k, L, scoring, weighting, nodes, words, device
extern "C" int cms_vocab_info(const cms_vocab* v, int* info) {
  if (!v || !info) return cms_fail(CMS_ERR_ARG, "cms_vocab_info: bad argument");
  const int o[7] = {v->dv.k, v->dv.L, v->dv.scoring, v->dv.weighting, v->dv.n_nodes, v->dv.n_words, v->device};
  std::memcpy(info, o, sizeof(o));
  return CMS_OK;
}

namespace {
// the arrays of one row behind each other (cap features); counts live elsewhere
struct VocRowLayout { size_t fw, fnid, wid, wval, nid, noff, nfeat, fnode, bytes; };
VocRowLayout voc_row_layout(int cap) {
  CmsBlock b;
  const size_t c = (size_t)std::max(cap, 1);
  VocRowLayout l;
  l.fw = b.take(4 * c); l.fnid = b.take(4 * c); l.wid = b.take(4 * c); l.wval = b.take(8 * c); l.nid = b.take(4 * c); l.noff = b.take(4 * (c + 1));
  l.nfeat = b.take(4 * c); l.fnode = b.take(4 * c); l.bytes = b.size;
  return l;
}
CmsVocRow voc_row_at(uint8_t* base, const VocRowLayout& l, const void* desc, int n, bool feat_node, int* counts) {
  CmsVocRow r;
  r.desc = (const uint32_t*)desc; r.n = n;
  r.feat_word = (int*)(base + l.fw); r.feat_nid = (int*)(base + l.fnid); r.word_id = (int*)(base + l.wid); r.word_val = (double*)(base + l.wval);
  r.node_id = (int*)(base + l.nid); r.node_off = (int*)(base + l.noff); r.node_feat = (int*)(base + l.nfeat);
  r.feat_node = feat_node ? (int*)(base + l.fnode) : nullptr; r.counts = counts;
  return r;
}
// developer aid (cms_vocab_profile_enable / _get, tools/prof_bow_transform.py): events around the two launches of the process's last call
struct VocProf { bool on = false, have = false; hipEvent_t ev[3] = {nullptr, nullptr, nullptr}; };
VocProf g_voc_prof;
// the two launches of a call; d_rows is on the device already (in stream order)
int voc_launch(const cms_vocab* v, hipStream_t s, const CmsVocRow* d_rows, int n_rows, int max_n, int levelsup) {
  const bool prof = g_voc_prof.on;
  if (prof) {
    for (hipEvent_t& e : g_voc_prof.ev) if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(g_voc_prof.ev[0], s));
  }
  if (max_n > 0) {
    const int per = CMS_VOC_THREADS / v->group;
    const dim3 grid((max_n + per - 1) / per, n_rows);
    if (v->group == 16) hipLaunchKernelGGL(k_vocab_descend<16>, grid, dim3(CMS_VOC_THREADS), 0, s, v->dv, d_rows, levelsup);
    else hipLaunchKernelGGL(k_vocab_descend<32>, grid, dim3(CMS_VOC_THREADS), 0, s, v->dv, d_rows, levelsup);
    HIPCHK(hipGetLastError());
  }
  if (prof) HIPCHK(hipEventRecord(g_voc_prof.ev[1], s));
  int P = CMS_VOC_THREADS;
  while (P < max_n) P <<= 1;
  static bool lds_done[64] = {};
  const int rc = cms_lds_ceiling_once((const void*)k_vocab_build, (CMS_AREA_MAXKP + 1) * 8, v->device, lds_done);
  if (rc) return rc;
  hipLaunchKernelGGL(k_vocab_build, dim3(n_rows), dim3(CMS_VOC_THREADS), (size_t)P * 8, s, v->dv, d_rows);
  HIPCHK(hipGetLastError());
  if (prof) { HIPCHK(hipEventRecord(g_voc_prof.ev[2], s)); g_voc_prof.have = true; }
  return CMS_OK;
}
int voc_check_call(const cms_vocab* v, int device, int levelsup, const char* who) {
  if (!v || levelsup < 0) return cms_fail(CMS_ERR_ARG, who);
  if (v->device != device) return cms_fail(CMS_ERR_ARG, "ComputeBoW: the vocabulary lives on another device");
  return CMS_OK;
}
}  // namespace

// Developer aid, one thread at a time: with profiling on, every ComputeBoW call of the process records events around its two launches;
// cms_vocab_profile_get (after the call has returned: the calls are synchronous) gives ms[0] = k_vocab_descend, ms[1] = k_vocab_build of the last one.
extern "C" int cms_vocab_profile_enable(int on) { g_voc_prof.on = on != 0; g_voc_prof.have = false; return CMS_OK; }
extern "C" int cms_vocab_profile_get(float* ms2) {
  if (!ms2 || !g_voc_prof.have) return cms_fail(CMS_ERR_ARG, "cms_vocab_profile_get: no profiled call");
  HIPCHK(hipEventElapsedTime(&ms2[0], g_voc_prof.ev[0], g_voc_prof.ev[1]));
  HIPCHK(hipEventElapsedTime(&ms2[1], g_voc_prof.ev[1], g_voc_prof.ev[2]));
  return CMS_OK;
}

// ---- stand-alone: descriptors from the host (n x 32 bytes).  word_id / word_val / node_id / node_feat hold up to n entries, node_off n + 1.
extern "C" int cms_vocab_transform(cms_vocab* v, cms_ctx* c, int n, const uint8_t* desc, int levelsup, int* nwords, int* word_id, double* word_val, int* nnodes,
                                   int* node_id, int* node_off, int* node_feat) {
  if (!c || n < 0 || !nwords || !nnodes || !node_off || (n > 0 && (!desc || !word_id || !word_val || !node_id || !node_feat)))
    return cms_fail(CMS_ERR_ARG, "cms_vocab_transform: bad argument");
  if (n > CMS_AREA_MAXKP) return cms_fail(CMS_ERR_UNSUPPORTED, "cms_vocab_transform: more than 16383 features");
  int rc = voc_check_call(v, c->device, levelsup, "cms_vocab_transform: bad argument");
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  const VocRowLayout l = voc_row_layout(n);
  CmsBlock blk;
  const size_t o_row = blk.take(sizeof(CmsVocRow)), o_desc = blk.take(32 * (size_t)n), in_bytes = blk.size;
  const size_t o_cnt = blk.take(16), o_out = blk.take(l.bytes);
  hipStream_t s = c->stream;
  rc = c->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* d = c->stage.d;
  uint8_t* h = c->stage.h;
  const CmsVocRow row = voc_row_at(d + o_out, l, d + o_desc, n, false, (int*)(d + o_cnt));
  std::memcpy(h + o_row, &row, sizeof(row));
  if (n > 0) std::memcpy(h + o_desc, desc, 32 * (size_t)n);
  rc = c->stage.up(s, in_bytes, "cms_vocab_transform");
  if (rc) return rc;
  rc = voc_launch(v, s, (const CmsVocRow*)(d + o_row), 1, n, levelsup);
  if (rc) return rc;
  rc = c->stage.back_and_wait(s, o_cnt, blk.size, "cms_vocab_transform");
  if (rc) return rc;
  const int* cnt = (const int*)(h + o_cnt);
  const uint8_t* o = h + o_out;
  *nwords = cnt[0]; *nnodes = cnt[1];
  if (cnt[0] > 0) { std::memcpy(word_id, o + l.wid, 4 * (size_t)cnt[0]); std::memcpy(word_val, o + l.wval, 8 * (size_t)cnt[0]); }
  if (cnt[1] > 0) std::memcpy(node_id, o + l.nid, 4 * (size_t)cnt[1]);
  std::memcpy(node_off, o + l.noff, 4 * ((size_t)cnt[1] + 1));
  if (cnt[2] > 0) std::memcpy(node_feat, o + l.nfeat, 4 * (size_t)cnt[2]);
  return CMS_OK;
}

// ---- frame rows: the descriptors cms_frames_process left on the device; the results stay resident per row
struct CmsCtxBow {
  int cap = 0, max_batch = 0;
  VocRowLayout l;
  uint8_t* d = nullptr; int* d_counts = nullptr; CmsVocRow* d_rows = nullptr;
  uint8_t* h = nullptr;      // pinned: the call's row table, then 3 counts per row of the context
  std::vector<int> n, nwords, nnodes, nfeat;      // n < 0: the row has no BoW
};
static void cms_ctx_bow_free(CmsCtxBow* b) {
  if (!b) return;
  if (b->d) (void)hipFree(b->d);
  if (b->d_counts) (void)hipFree(b->d_counts);
  if (b->d_rows) (void)hipFree(b->d_rows);
  if (b->h) (void)hipHostFree(b->h);
  delete b;
}
static void cms_ctx_bow_invalidate(CmsCtxBow* b) {
  if (b) std::fill(b->n.begin(), b->n.end(), -1);
}
static int cms_ctx_bow_reserve(cms_ctx* c) {
  if (c->bow) return CMS_OK;
  CmsCtxBow* b = new CmsCtxBow();
  b->cap = std::min(c->g.kp_cap, (int)CMS_AREA_MAXKP); b->max_batch = c->max_batch;
  b->l = voc_row_layout(b->cap);
  const size_t B = (size_t)c->max_batch;
  if (hipMalloc((void**)&b->d, B * b->l.bytes) != hipSuccess || hipMalloc((void**)&b->d_counts, B * 12) != hipSuccess ||
      hipMalloc((void**)&b->d_rows, B * sizeof(CmsVocRow)) != hipSuccess || hipHostMalloc((void**)&b->h, B * (sizeof(CmsVocRow) + 12)) != hipSuccess) {
    cms_ctx_bow_free(b);
    return cms_fail(CMS_ERR_HIP, "cms_frames_compute_bow: out of memory");
  }
  b->n.assign(B, -1); b->nwords.assign(B, 0); b->nnodes.assign(B, 0); b->nfeat.assign(B, 0);
  c->bow = b;
  return CMS_OK;
}
static CmsVocRow cms_ctx_bow_row(cms_ctx* c, int b, int n) {
  CmsCtxBow* w = c->bow;
  return voc_row_at(w->d + (size_t)b * w->l.bytes, w->l, c->d_desc + 32 * (size_t)b * c->g.kp_cap, n, false, w->d_counts + 3 * (size_t)b);
}

extern "C" int cms_frames_compute_bow(cms_ctx* c, cms_vocab* v, int levelsup, int n_rows, const int* rows, const int* n) {
  if (!c || n_rows < 0 || (n_rows > 0 && (!rows || !n))) return cms_fail(CMS_ERR_ARG, "cms_frames_compute_bow: bad argument");
  int rc = voc_check_call(v, c->device, levelsup, "cms_frames_compute_bow: bad argument");
  if (rc) return rc;
  std::vector<uint8_t> seen((size_t)c->max_batch, 0);
  int max_n = 0;
  for (int i = 0; i < n_rows; ++i) {
    if (rows[i] < 0 || rows[i] >= c->max_batch || n[i] < 0) return cms_fail(CMS_ERR_ARG, "cms_frames_compute_bow: bad frame row or count");
    if (n[i] > CMS_AREA_MAXKP) return cms_fail(CMS_ERR_UNSUPPORTED, "cms_frames_compute_bow: more than 16383 key points in a frame");
    if (n[i] > c->g.kp_cap) return cms_fail(CMS_ERR_ARG, "cms_frames_compute_bow: more key points than a frame row of the context holds");
    if (seen[(size_t)rows[i]]) return cms_fail(CMS_ERR_ARG, "cms_frames_compute_bow: a row is named twice");
    seen[(size_t)rows[i]] = 1;
    max_n = std::max(max_n, n[i]);
  }
  if (n_rows == 0) return CMS_OK;
  HIPCHK(hipSetDevice(c->device));
  rc = cms_ctx_bow_reserve(c);
  if (rc) return rc;
  CmsCtxBow* w = c->bow;
  CmsVocRow* hr = reinterpret_cast<CmsVocRow*>(w->h);
  int* hc = reinterpret_cast<int*>(w->h + (size_t)c->max_batch * sizeof(CmsVocRow));
  for (int i = 0; i < n_rows; ++i) { hr[i] = cms_ctx_bow_row(c, rows[i], n[i]); w->n[(size_t)rows[i]] = -1; }
  hipStream_t s = c->stream;
  HIPCHK(hipMemcpyAsync(w->d_rows, hr, (size_t)n_rows * sizeof(CmsVocRow), hipMemcpyHostToDevice, s));
  rc = voc_launch(v, s, w->d_rows, n_rows, max_n, levelsup);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(hc, w->d_counts, (size_t)c->max_batch * 12, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int i = 0; i < n_rows; ++i) {
    const size_t b = (size_t)rows[i];
    w->n[b] = n[i]; w->nwords[b] = hc[3 * b]; w->nnodes[b] = hc[3 * b + 1]; w->nfeat[b] = hc[3 * b + 2];
  }
  return CMS_OK;
}

// what the host needs for mBowVec, mFeatVec and the key-frame database.  The counts are always delivered; arrays that a capacity cannot hold make
// the call CMS_ERR_OVERFLOW with nothing copied (node_off needs node_cap + 1 entries).
extern "C" int cms_frames_fetch_bow(cms_ctx* c, int b, int* nwords, int* word_id, double* word_val, int word_cap, int* nnodes, int* node_id, int* node_off,
                                    int* node_feat, int node_cap, int feat_cap) {
  if (!c || !nwords || !nnodes || b < 0 || b >= c->max_batch || word_cap < 0 || node_cap < 0 || feat_cap < 0)
    return cms_fail(CMS_ERR_ARG, "cms_frames_fetch_bow: bad argument");
  CmsCtxBow* w = c->bow;
  if (!w || w->n[(size_t)b] < 0) return cms_fail(CMS_ERR_ARG, "cms_frames_fetch_bow: no BoW computed for this row (cms_frames_compute_bow first)");
  const int nw = w->nwords[(size_t)b], nn = w->nnodes[(size_t)b], nf = w->nfeat[(size_t)b];
  *nwords = nw; *nnodes = nn;
  if (nw > word_cap || nn > node_cap || nf > feat_cap) return cms_fail(CMS_ERR_OVERFLOW, "cms_frames_fetch_bow: a capacity is too small");
  if ((nw > 0 && (!word_id || !word_val)) || !node_off || (nn > 0 && !node_id) || (nf > 0 && !node_feat)) return cms_fail(CMS_ERR_ARG, "cms_frames_fetch_bow: null array");
  HIPCHK(hipSetDevice(c->device));
  const CmsVocRow r = cms_ctx_bow_row(c, b, w->n[(size_t)b]);
  hipStream_t s = c->stream;
  if (nw > 0) { HIPCHK(hipMemcpyAsync(word_id, r.word_id, 4 * (size_t)nw, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(word_val, r.word_val, 8 * (size_t)nw, hipMemcpyDeviceToHost, s)); }
  if (nn > 0) HIPCHK(hipMemcpyAsync(node_id, r.node_id, 4 * (size_t)nn, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(node_off, r.node_off, 4 * ((size_t)nn + 1), hipMemcpyDeviceToHost, s));
  if (nf > 0) HIPCHK(hipMemcpyAsync(node_feat, r.node_feat, 4 * (size_t)nf, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return CMS_OK;
}

// ---- resident key frames: KeyFrame::ComputeBoW on the slots' descriptors.  The vectors are computed into scratch first: a slot is written only
// when every slot of the call fits the store's max_nodes.
struct CmsStoreBow {
  int* d_word_id = nullptr; double* d_word_val = nullptr; int* d_nwords = nullptr;      // BowVector per slot (max_features entries)
  CmsStage tmp;      // the call's scratch (row table | commit records | counts | rows) and the pinned copy of its head
  std::vector<int> nwords, nfeat;      // nwords < 0: the slot has no BowVector; nfeat: features its FeatureVector lists
};
static void cms_store_bow_free(CmsStoreBow* b) {
  if (!b) return;
  void* bufs[] = {b->d_word_id, b->d_word_val, b->d_nwords};
  for (void* p : bufs) if (p) (void)hipFree(p);
  b->tmp.release();
  delete b;
}

static void cms_store_bow_invalidate(CmsStoreBow* b, int slot) {
  if (b) b->nwords[(size_t)slot] = -1;
}

// the slots' BowVector arrays, allocated by the first call that gives a slot one (cms_kfstore_compute_bow, cms_kfstore_set_bow)
static int cms_store_bow_reserve(cms_kfstore* st, const char* oom) {
  if (st->bow) return CMS_OK;
  const size_t K = (size_t)st->maxkf, Fq = (size_t)st->maxf;
  CmsStoreBow* b = new CmsStoreBow();
  if (hipMalloc((void**)&b->d_word_id, K * Fq * 4) != hipSuccess || hipMalloc((void**)&b->d_word_val, K * Fq * 8) != hipSuccess ||
      hipMalloc((void**)&b->d_nwords, K * 4) != hipSuccess) {
    cms_store_bow_free(b);
    return cms_fail(CMS_ERR_HIP, oom);
  }
  b->nwords.assign(K, -1); b->nfeat.assign(K, 0);
  st->bow = b;
  return CMS_OK;
}

extern "C" int cms_kfstore_compute_bow(cms_kfstore* st, cms_vocab* v, int levelsup, int n_slots, const int* slots) {
  if (!st || n_slots < 0 || n_slots > st->maxkf || (n_slots > 0 && !slots)) return cms_fail(CMS_ERR_ARG, "cms_kfstore_compute_bow: bad argument");
  cms_ctx* c = st->c;
  int rc = voc_check_call(v, c->device, levelsup, "cms_kfstore_compute_bow: bad argument");
  if (rc) return rc;
  {
    std::vector<uint8_t> seen((size_t)st->maxkf, 0);
    for (int i = 0; i < n_slots; ++i) {
      if (slots[i] < 0 || slots[i] >= st->maxkf || !st->used[(size_t)slots[i]]) return cms_fail(CMS_ERR_ARG, "cms_kfstore_compute_bow: empty slot");
      if (seen[(size_t)slots[i]]) return cms_fail(CMS_ERR_ARG, "cms_kfstore_compute_bow: a slot is named twice");
      seen[(size_t)slots[i]] = 1;
    }
  }
  if (n_slots == 0) return CMS_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(kfstore_order_behind_puts(st));
  const size_t Fq = (size_t)st->maxf, S = (size_t)n_slots;
  rc = cms_store_bow_reserve(st, "cms_kfstore_compute_bow: out of device memory");
  if (rc) return rc;
  CmsStoreBow* w = st->bow;
  const VocRowLayout l = voc_row_layout(st->maxf);
  CmsBlock blk;
  const size_t o_rows = blk.take(S * sizeof(CmsVocRow)), o_commit = blk.take(S * sizeof(CmsVocCommit)), in_bytes = blk.size;
  const size_t o_cnt = blk.take(S * 12), head_bytes = blk.size, o_out = blk.take(S * l.bytes);
  hipStream_t s = c->stream;
  rc = w->tmp.reserve(s, blk.size, head_bytes);
  if (rc) return rc;
  uint8_t* d = w->tmp.d;
  uint8_t* h = w->tmp.h;
  CmsVocRow* hr = reinterpret_cast<CmsVocRow*>(h + o_rows);
  CmsVocCommit* hcm = reinterpret_cast<CmsVocCommit*>(h + o_commit);
  int max_n = 0;
  for (int i = 0; i < n_slots; ++i) {
    const CmsTriKF& k = st->h_kf[(size_t)slots[i]];
    const size_t f0 = (size_t)k.f0;
    hr[i] = voc_row_at(d + o_out + (size_t)i * l.bytes, l, st->d_desc + 32 * f0, k.n, true, (int*)(d + o_cnt) + 3 * (size_t)i);
    CmsVocCommit& cm = hcm[i];
    cm.src = hr[i];
    cm.o_fn = st->d_fn + f0; cm.o_nid = st->d_nid + k.node0; cm.o_noff = st->d_noff + k.noff0; cm.o_nfeat = st->d_nfeat + k.nfeat0;
    cm.o_kf_nnodes = &st->d_kf[slots[i]].nnodes;
    cm.o_word_id = w->d_word_id + (size_t)slots[i] * Fq; cm.o_word_val = w->d_word_val + (size_t)slots[i] * Fq; cm.o_nwords = w->d_nwords + slots[i];
    max_n = std::max(max_n, k.n);
  }
  rc = w->tmp.up(s, in_bytes, "cms_kfstore_compute_bow");
  if (rc) return rc;
  rc = voc_launch(v, s, (const CmsVocRow*)(d + o_rows), n_slots, max_n, levelsup);
  if (rc) return rc;
  rc = w->tmp.back_and_wait(s, o_cnt, o_cnt + S * 12, "cms_kfstore_compute_bow");
  if (rc) return rc;
  const int* cnt = reinterpret_cast<const int*>(h + o_cnt);
  for (int i = 0; i < n_slots; ++i)
    if (cnt[3 * i + 1] > st->maxn) return cms_fail(CMS_ERR_OVERFLOW, "cms_kfstore_compute_bow: a FeatureVector has more nodes than the store's max_nodes (no slot was changed)");
  hipLaunchKernelGGL(k_vocab_commit, dim3(n_slots), dim3(CMS_VOC_THREADS), 0, s, (const CmsVocCommit*)(d + o_commit));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  for (int i = 0; i < n_slots; ++i) { st->h_kf[(size_t)slots[i]].nnodes = cnt[3 * i + 1]; w->nwords[(size_t)slots[i]] = cnt[3 * i]; w->nfeat[(size_t)slots[i]] = cnt[3 * i + 2]; }
  return CMS_OK;
}

// The slot's BowVector and, when node_off is given, its FeatureVector as the call computed it (what KeyFrame::mBowVec / mFeatVec hold).  The counts
// are always delivered; a capacity that cannot hold its array is CMS_ERR_OVERFLOW with nothing copied (node_off needs node_cap + 1 entries).
extern "C" int cms_kfstore_fetch_bow(cms_kfstore* st, int slot, int* nwords, int* word_id, double* word_val, int word_cap, int* nnodes, int* node_id, int* node_off,
                                     int* node_feat, int node_cap, int feat_cap) {
  if (!st || !nwords || slot < 0 || slot >= st->maxkf || !st->used[(size_t)slot] || word_cap < 0 || node_cap < 0 || feat_cap < 0)
    return cms_fail(CMS_ERR_ARG, "cms_kfstore_fetch_bow: bad argument");
  CmsStoreBow* w = st->bow;
  if (!w || w->nwords[(size_t)slot] < 0) return cms_fail(CMS_ERR_ARG, "cms_kfstore_fetch_bow: no BowVector computed for this slot (cms_kfstore_compute_bow first)");
  const CmsTriKF& k = st->h_kf[(size_t)slot];
  const int nw = w->nwords[(size_t)slot], nn = k.nnodes, nf = w->nfeat[(size_t)slot];
  *nwords = nw;
  if (nnodes) *nnodes = nn;
  const bool fv = node_off != nullptr;
  if (nw > word_cap || (fv && (nn > node_cap || nf > feat_cap))) return cms_fail(CMS_ERR_OVERFLOW, "cms_kfstore_fetch_bow: a capacity is too small");
  if ((nw > 0 && (!word_id || !word_val)) || (fv && ((nn > 0 && !node_id) || (nf > 0 && !node_feat)))) return cms_fail(CMS_ERR_ARG, "cms_kfstore_fetch_bow: null array");
  cms_ctx* c = st->c;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(kfstore_order_behind_puts(st));
  hipStream_t s = c->stream;
  if (nw > 0) {
    HIPCHK(hipMemcpyAsync(word_id, w->d_word_id + (size_t)slot * st->maxf, 4 * (size_t)nw, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(word_val, w->d_word_val + (size_t)slot * st->maxf, 8 * (size_t)nw, hipMemcpyDeviceToHost, s));
  }
  if (fv) {
    if (nn > 0) HIPCHK(hipMemcpyAsync(node_id, st->d_nid + k.node0, 4 * (size_t)nn, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(node_off, st->d_noff + k.noff0, 4 * ((size_t)nn + 1), hipMemcpyDeviceToHost, s));
    if (nf > 0) HIPCHK(hipMemcpyAsync(node_feat, st->d_nfeat + k.nfeat0, 4 * (size_t)nf, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return CMS_OK;
}

// Relocalization's candidate loop (Tracking.cpp:1019-1040) or one TrackReferenceKeyFrame per camera stream on resident key frames: ONE launch on
// src's stream.  Nothing is enqueued on the store's stream; the copies of cms_kfstore_put_from_frame(s) that filled a named slot are waited for on
// the device (their events: the copy may still be in flight when it ran on another context's stream).
// frames: cms_kfstore_search_by_bow_frames -- the frame side's FeatureVector is taken from the row's resident result (the jobs' node arrays are not read)
static int kfstore_search_by_bow_run(cms_kfstore* st, cms_ctx* src, int njobs, const cms_bow_job* jobs, float nnratio, int check_orientation, int* kf_idx,
                                     int* n_matches, bool frames) {
  const std::string who = frames ? "cms_kfstore_search_by_bow_frames" : "cms_kfstore_search_by_bow";
  if (!st || !src || njobs < 0 || (njobs > 0 && (!jobs || !n_matches))) return cms_fail(CMS_ERR_ARG, (who + ": bad argument").c_str());
  if (njobs == 0) return CMS_OK;
  if (src->device != st->c->device) return cms_fail(CMS_ERR_ARG, (who + ": the frame context and the store must share the device").c_str());
  std::vector<uint8_t> seen;
  size_t total_n = 0;
  for (int j = 0; j < njobs; ++j) {
    const cms_bow_job& q = jobs[j];
    if (q.slot < 0 || q.slot >= st->maxkf || !st->used[(size_t)q.slot]) return cms_fail(CMS_ERR_ARG, (who + ": empty slot").c_str());
    int rc = bow_check_frame(src, q.b, q.n, (who + ": bad frame").c_str());
    if (rc) return rc;
    if (frames) {
      if (!src->bow || src->bow->n[(size_t)q.b] < 0) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_bow_frames: no BoW computed for the frame row (cms_frames_compute_bow first)");
      if (src->bow->n[(size_t)q.b] != q.n) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_bow_frames: the row's BoW was computed for another key-point count");
    } else {
      rc = bow_check_fv(q.n, q.nnodes, q.node_id, q.node_off, q.node_feat, &seen, "cms_kfstore_search_by_bow: bad frame FeatureVector");
      if (rc) return rc;
    }
    total_n += (size_t)q.n;
  }
  if (total_n > 0 && !kf_idx) return cms_fail(CMS_ERR_ARG, (who + ": bad argument").c_str());
  HIPCHK(hipSetDevice(src->device));
  int rc = kfstore_wait_puts(st, src->stream, njobs, [&](int j) { return jobs[j].slot; });
  if (rc) return rc;
  std::vector<CmsBowJob> dj((size_t)njobs);
  std::vector<std::vector<const void**>> rel((size_t)njobs);
  std::vector<BowStage> pieces;
  CmsBlock blk;
  for (int j = 0; j < njobs; ++j) {
    const cms_bow_job& q = jobs[j];
    const CmsTriKF& k = st->h_kf[(size_t)q.slot];
    CmsBowJob& d = dj[(size_t)j];
    std::memset(&d, 0, sizeof(d));
    d.kf_kp = st->d_kp + k.f0; d.kf_desc = (const uint4*)(st->d_desc + 32 * (size_t)k.f0); d.kf_mp = st->d_mp + k.f0;
    d.kf_nid = st->d_nid + k.node0; d.kf_noff = st->d_noff + k.noff0; d.kf_nfeat = st->d_nfeat + k.nfeat0; d.kf_nnodes = k.nnodes;
    if (q.kf_skip) bow_put(pieces, blk, rel[(size_t)j], d.kf_skip, q.kf_skip, (size_t)k.n);
    if (frames) {
      const CmsVocRow r = cms_ctx_bow_row(src, q.b, q.n);
      d.f_nid = r.node_id; d.f_noff = r.node_off; d.f_nfeat = r.node_feat; d.f_nnodes = src->bow->nnodes[(size_t)q.b];
    } else {
      const int ffeat = q.nnodes > 0 ? q.node_off[q.nnodes] : 0;
      bow_put(pieces, blk, rel[(size_t)j], d.f_nid, q.node_id, 4 * (size_t)q.nnodes);
      bow_put(pieces, blk, rel[(size_t)j], d.f_noff, q.node_off, q.nnodes > 0 ? 4 * ((size_t)q.nnodes + 1) : 0);
      bow_put(pieces, blk, rel[(size_t)j], d.f_nfeat, q.node_feat, 4 * (size_t)ffeat);
      d.f_nnodes = q.nnodes;
    }
    d.n = q.n;
    const size_t sb = (size_t)q.b * src->g.kp_cap;
    d.f_kp = (const CmsKeyPoint*)src->d_kps + sb; d.f_desc = (const uint4*)(src->d_desc + 32 * sb);
  }
  return bow_run(src, dj, rel, pieces, blk, nnratio, check_orientation, kf_idx, n_matches, who.c_str());
}
extern "C" int cms_kfstore_search_by_bow(cms_kfstore* st, cms_ctx* src, int njobs, const cms_bow_job* jobs, float nnratio, int check_orientation,
                                         int* kf_idx, int* n_matches) {
  return kfstore_search_by_bow_run(st, src, njobs, jobs, nnratio, check_orientation, kf_idx, n_matches, false);
}
extern "C" int cms_kfstore_search_by_bow_frames(cms_kfstore* st, cms_ctx* src, int njobs, const cms_bow_job* jobs, float nnratio, int check_orientation,
                                                int* kf_idx, int* n_matches) {
  return kfstore_search_by_bow_run(st, src, njobs, jobs, nnratio, check_orientation, kf_idx, n_matches, true);
}
