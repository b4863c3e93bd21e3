// cms_api_kfdb.hip -- host side of KeyFrameDatabase (src/KeyFrameDatabase.cpp) over the resident key frames of a cms_kfstore: the database's table
// (membership, group, add sequence number, covisibles per slot) lives on the host under one mutex, the BowVectors are the store's
// (CmsStoreBow), reloc_score lives on the device only.  Included by cms_lib.hip behind cms_api_vocab.hip and cms_kfdb_kernels.hip.
// cms_kfdb_detect takes a snapshot of the table under the mutex and uploads it with the call: ONE upload, k_kfdb_common / k_kfdb_score / k_kfdb_carry /
// k_kfdb_select on the caller's stream, ONE copy back, ONE wait (CmsStage).
#include <cstring>
#include <vector>

struct CmsStoreKfdb {
  std::mutex mu;                // the table: add / erase / clear / set_covisibles / refill on the mapping thread, the snapshot on the frame thread
  std::vector<uint8_t> in_db, reset;      // reset: added since the last detect read the slot's reloc_score (it starts at 0.0f)
  std::vector<int> group, nwords, covis;  // nwords: the BowVector's length when the slot was added
  std::vector<unsigned long long> seq;
  unsigned long long next_seq = 0;
  std::mutex detect_mu;         // one cms_kfdb_detect per store at a time: the stage and the slots' reloc_score
  CmsStage stage;
  float* d_reloc = nullptr;
};
static CmsStoreKfdb* cms_store_kfdb_new(int max_keyframes) {
  CmsStoreKfdb* d = new CmsStoreKfdb();
  const size_t K = (size_t)max_keyframes;
  d->in_db.assign(K, 0); d->reset.assign(K, 0); d->group.assign(K, 0); d->nwords.assign(K, 0); d->covis.assign(K * CMS_KFDB_COVIS, -1); d->seq.assign(K, 0);
  if (hipMalloc((void**)&d->d_reloc, K * 4) != hipSuccess || hipMemset(d->d_reloc, 0, K * 4) != hipSuccess) { if (d->d_reloc) (void)hipFree(d->d_reloc); delete d; return nullptr; }
  return d;
}
static void cms_store_kfdb_free(CmsStoreKfdb* d) {
  if (!d) return;
  if (d->d_reloc) (void)hipFree(d->d_reloc);
  d->stage.release();
  delete d;
}
static void cms_store_kfdb_refill(CmsStoreKfdb* d, int slot) {
  if (!d) return;
  std::lock_guard<std::mutex> lk(d->mu);
  d->in_db[(size_t)slot] = 0;
  std::fill(d->covis.begin() + (size_t)slot * CMS_KFDB_COVIS, d->covis.begin() + ((size_t)slot + 1) * CMS_KFDB_COVIS, -1);
}

static bool kfdb_slot_has_bow(const cms_kfstore* st, int slot) {
  return slot >= 0 && slot < st->maxkf && st->used[(size_t)slot] && st->bow && st->bow->nwords[(size_t)slot] >= 0;
}

// The BowVector the host computed for the key frame in `slot` (a key frame put with a host-computed FeatureVector has none otherwise).  On the store's
// stream, synchronous.
extern "C" int cms_kfstore_set_bow(cms_kfstore* st, int slot, int nwords, const int* word_id, const double* word_val) {
  if (!st || slot < 0 || slot >= st->maxkf || !st->used[(size_t)slot] || nwords < 0 || (nwords > 0 && (!word_id || !word_val)))
    return cms_fail(CMS_ERR_ARG, "cms_kfstore_set_bow: bad argument or empty slot");
  if (nwords > st->maxf) return cms_fail(CMS_ERR_ARG, "cms_kfstore_set_bow: more words than the store's max_features");
  if (!cms_kfdb_bow_ok(nwords, word_id)) return cms_fail(CMS_ERR_ARG, "cms_kfstore_set_bow: word ids must be >= 0 and strictly ascending");
  { std::lock_guard<std::mutex> lk(st->kfdb->mu); if (st->kfdb->in_db[(size_t)slot]) return cms_fail(CMS_ERR_ARG, "cms_kfstore_set_bow: the slot is in the database (cms_kfdb_erase first)"); }
  cms_ctx* c = st->c;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(kfstore_order_behind_puts(st));
  const int rc = cms_store_bow_reserve(st, "cms_kfstore_set_bow: out of device memory");
  if (rc) return rc;
  CmsStoreBow* w = st->bow;
  hipStream_t s = c->stream;
  if (nwords > 0) {
    HIPCHK(hipMemcpyAsync(w->d_word_id + (size_t)slot * st->maxf, word_id, 4 * (size_t)nwords, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w->d_word_val + (size_t)slot * st->maxf, word_val, 8 * (size_t)nwords, hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipMemcpyAsync(w->d_nwords + slot, &nwords, 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  w->nwords[(size_t)slot] = nwords;
  return CMS_OK;
}

// KeyFrameDatabase::add (LoopClosing.cpp:115, :145, :214): all slots of the call or none
extern "C" int cms_kfdb_add(cms_kfstore* st, int n, const int* slots, const int* groups) {
  if (!st || n < 0 || (n > 0 && (!slots || !groups))) return cms_fail(CMS_ERR_ARG, "cms_kfdb_add: bad argument");
  CmsStoreKfdb* d = st->kfdb;
  std::lock_guard<std::mutex> lk(d->mu);
  for (int i = 0; i < n; ++i) {
    if (groups[i] < 0) return cms_fail(CMS_ERR_ARG, "cms_kfdb_add: negative group");
    if (!kfdb_slot_has_bow(st, slots[i])) return cms_fail(CMS_ERR_ARG, "cms_kfdb_add: a slot is empty or has no BowVector (cms_kfstore_compute_bow or cms_kfstore_set_bow first)");
    if (d->in_db[(size_t)slots[i]]) return cms_fail(CMS_ERR_ARG, "cms_kfdb_add: a slot is in the database already");
    for (int j = 0; j < i; ++j) if (slots[j] == slots[i]) return cms_fail(CMS_ERR_ARG, "cms_kfdb_add: a slot is named twice");
  }
  for (int i = 0; i < n; ++i) {
    const size_t s = (size_t)slots[i];
    d->in_db[s] = 1; d->reset[s] = 1; d->group[s] = groups[i]; d->nwords[s] = st->bow->nwords[s]; d->seq[s] = d->next_seq++;
  }
  return CMS_OK;
}
// KeyFrameDatabase::erase (KeyFrame.cpp:569): a slot that is not in the database is left alone, as in the reference
extern "C" int cms_kfdb_erase(cms_kfstore* st, int n, const int* slots) {
  if (!st || n < 0 || (n > 0 && !slots)) return cms_fail(CMS_ERR_ARG, "cms_kfdb_erase: bad argument");
  for (int i = 0; i < n; ++i) if (slots[i] < 0 || slots[i] >= st->maxkf) return cms_fail(CMS_ERR_ARG, "cms_kfdb_erase: bad slot");
  std::lock_guard<std::mutex> lk(st->kfdb->mu);
  for (int i = 0; i < n; ++i) st->kfdb->in_db[(size_t)slots[i]] = 0;
  return CMS_OK;
}
// KeyFrameDatabase::clear (Tracking.cpp:1176) for one group, or for all with group = -1
extern "C" int cms_kfdb_clear(cms_kfstore* st, int group) {
  if (!st || group < -1) return cms_fail(CMS_ERR_ARG, "cms_kfdb_clear: bad argument");
  CmsStoreKfdb* d = st->kfdb;
  std::lock_guard<std::mutex> lk(d->mu);
  for (size_t s = 0; s < d->in_db.size(); ++s) if (group < 0 || d->group[s] == group) d->in_db[s] = 0;
  return CMS_OK;
}
// GetBestCovisibilityKeyFrames(10) of the key frames in `slots` as slots, best first, padded with -1: all of the call or none
extern "C" int cms_kfdb_set_covisibles(cms_kfstore* st, int n, const int* slots, const int* neigh) {
  if (!st || n < 0 || (n > 0 && (!slots || !neigh))) return cms_fail(CMS_ERR_ARG, "cms_kfdb_set_covisibles: bad argument");
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= st->maxkf) return cms_fail(CMS_ERR_ARG, "cms_kfdb_set_covisibles: bad slot");
    for (int c = 0; c < CMS_KFDB_COVIS; ++c)
      if (neigh[i * CMS_KFDB_COVIS + c] < -1 || neigh[i * CMS_KFDB_COVIS + c] >= st->maxkf) return cms_fail(CMS_ERR_ARG, "cms_kfdb_set_covisibles: bad covisible slot");
  }
  std::lock_guard<std::mutex> lk(st->kfdb->mu);
  for (int i = 0; i < n; ++i) std::copy(neigh + (size_t)i * CMS_KFDB_COVIS, neigh + ((size_t)i + 1) * CMS_KFDB_COVIS, st->kfdb->covis.begin() + (size_t)slots[i] * CMS_KFDB_COVIS);
  return CMS_OK;
}

// Developer aid (tools/prof_kfdb.py), one thread at a time: events around the launch sequence of the process's last cms_kfdb_detect
namespace { struct KfdbProf { bool on = false, have = false; hipEvent_t ev[2] = {nullptr, nullptr}; } g_kfdb_prof; }
extern "C" int cms_kfdb_profile_enable(int on) { g_kfdb_prof.on = on != 0; g_kfdb_prof.have = false; return CMS_OK; }
extern "C" int cms_kfdb_profile_get(float* ms) {
  if (!ms || !g_kfdb_prof.have) return cms_fail(CMS_ERR_ARG, "cms_kfdb_profile_get: no profiled call");
  HIPCHK(hipEventElapsedTime(ms, g_kfdb_prof.ev[0], g_kfdb_prof.ev[1]));
  return CMS_OK;
}

extern "C" int cms_kfdb_detect(cms_kfstore* st, cms_ctx* src, int njobs, const cms_kfdb_job* jobs, int cand_cap, int* cand_slot, int* n_cand, int* diag_common,
                               float* diag_score) {
  if (!st || !src || njobs < 0 || cand_cap < 0 || (njobs > 0 && (!jobs || !n_cand || (cand_cap > 0 && !cand_slot)))) return cms_fail(CMS_ERR_ARG, "cms_kfdb_detect: bad argument");
  if (njobs == 0) return CMS_OK;
  if (src->device != st->c->device) return cms_fail(CMS_ERR_ARG, "cms_kfdb_detect: the frame context and the store must share the device");
  const size_t K = (size_t)st->maxkf, Q = (size_t)njobs;
  size_t n_explicit = 0, n_conn = 0;
  int max_q = 0;
  for (int j = 0; j < njobs; ++j) {
    const cms_kfdb_job& q = jobs[j];
    if ((q.mode != CMS_KFDB_RELOC && q.mode != CMS_KFDB_LOOP) || q.group < 0) return cms_fail(CMS_ERR_ARG, "cms_kfdb_detect: bad mode or group");
    int nq = 0;
    if (q.query == CMS_KFDB_QUERY_ROW) {
      if (q.b < 0 || q.b >= src->max_batch || !src->bow || src->bow->n[(size_t)q.b] < 0)
        return cms_fail(CMS_ERR_ARG, "cms_kfdb_detect: no BoW computed for the frame row (cms_frames_compute_bow first)");
      nq = src->bow->nwords[(size_t)q.b];
    } else if (q.query == CMS_KFDB_QUERY_SLOT) {
      if (!kfdb_slot_has_bow(st, q.slot)) return cms_fail(CMS_ERR_ARG, "cms_kfdb_detect: the query slot is empty or has no BowVector");
      nq = st->bow->nwords[(size_t)q.slot];
    } else if (q.query == CMS_KFDB_QUERY_WORDS) {
      if (q.nwords < 0 || q.nwords > CMS_AREA_MAXKP || (q.nwords > 0 && (!q.word_id || !q.word_val)) || !cms_kfdb_bow_ok(q.nwords, q.word_id))
        return cms_fail(CMS_ERR_ARG, "cms_kfdb_detect: a query's words must be at most 16383, >= 0 and strictly ascending");
      nq = q.nwords; n_explicit += cms_align(8 * (size_t)nq) + cms_align(4 * (size_t)nq);
    } else return cms_fail(CMS_ERR_ARG, "cms_kfdb_detect: bad query form");
    max_q = std::max(max_q, nq);
    if (q.mode == CMS_KFDB_LOOP) {
      if (!(q.min_score == q.min_score) || q.n_connected < 0 || (q.n_connected > 0 && !q.connected)) return cms_fail(CMS_ERR_ARG, "cms_kfdb_detect: bad loop job");
      for (int i = 0; i < q.n_connected; ++i) if (q.connected[i] < 0 || q.connected[i] >= st->maxkf) return cms_fail(CMS_ERR_ARG, "cms_kfdb_detect: bad connected slot");
      n_conn += cms_align(4 * (size_t)q.n_connected);
    }
  }
  HIPCHK(hipSetDevice(src->device));
  CmsStoreKfdb* db = st->kfdb;
  std::lock_guard<std::mutex> call_lock(db->detect_mu);
  // ---- the snapshot: the database's slots in add order
  std::vector<int> order, rank(K, -1);
  std::vector<CmsKfdbDevEntry> ent;
  std::vector<int> covis;
  {
    std::lock_guard<std::mutex> lk(db->mu);
    for (size_t s = 0; s < K; ++s) if (db->in_db[s]) order.push_back((int)s);
    if (order.size() > CMS_KFDB_MAX_ENTRIES) return cms_fail(CMS_ERR_UNSUPPORTED, "cms_kfdb_detect: more than 16384 key frames in the database");
    std::sort(order.begin(), order.end(), [&](int a, int b) { return db->seq[(size_t)a] < db->seq[(size_t)b]; });
    ent.resize(order.size()); covis.resize(order.size() * CMS_KFDB_COVIS);
    for (size_t e = 0; e < order.size(); ++e) rank[(size_t)order[e]] = (int)e;
    for (size_t e = 0; e < order.size(); ++e) {
      const size_t s = (size_t)order[e];
      ent[e] = CmsKfdbDevEntry{(int)s, db->group[s], db->nwords[s], db->reset[s]};
      db->reset[s] = 0;
      for (int c = 0; c < CMS_KFDB_COVIS; ++c) { const int nb = db->covis[s * CMS_KFDB_COVIS + (size_t)c]; covis[e * CMS_KFDB_COVIS + (size_t)c] = nb < 0 ? -1 : rank[(size_t)nb]; }
    }
  }
  const size_t E = ent.size();
  if (diag_common) std::fill(diag_common, diag_common + Q * K, 0);
  if (diag_score) std::fill(diag_score, diag_score + Q * K, -1.0f);
  std::fill(n_cand, n_cand + Q, 0);
  if (E == 0) return CMS_OK;      // lKFsSharingWords.empty() (:112, :229)
  // the stored BowVectors were written by synchronous calls on the store's stream (cms_kfstore_compute_bow / cms_kfstore_set_bow, themselves ordered
  // behind the puts); what may still be in flight is a put of a query slot's key frame on another context's stream
  std::vector<int> query_slots;
  for (int j = 0; j < njobs; ++j) if (jobs[j].query == CMS_KFDB_QUERY_SLOT) query_slots.push_back(jobs[j].slot);
  int rc = kfstore_wait_puts(st, src->stream, (int)query_slots.size(), [&](int j) { return query_slots[(size_t)j]; });
  if (rc) return rc;
  // ---- one block: what goes up | what comes back | work
  const bool diag = diag_common || diag_score;
  CmsBlock blk;
  const size_t o_q = blk.take(Q * sizeof(CmsKfdbDevQuery)), o_ent = blk.take(E * sizeof(CmsKfdbDevEntry)), o_cov = blk.take(4 * E * CMS_KFDB_COVIS);
  const size_t o_var = blk.take(n_explicit + n_conn), o_maxc = blk.take(4 * Q), in_bytes = blk.size;
  const size_t o_ncand = blk.take(4 * Q), o_cand = blk.take(4 * Q * (size_t)cand_cap), out_end = blk.size;
  const size_t o_common = blk.take(4 * Q * E), o_score = blk.take(4 * Q * E), diag_end = blk.size;
  const size_t o_first = blk.take(4 * Q * E), o_seen = blk.take(4 * Q * E), o_fpos = blk.take(4 * Q * E);
  const size_t back_end = diag ? diag_end : out_end;
  hipStream_t s = src->stream;
  rc = db->stage.reserve(s, blk.size, back_end);
  if (rc) return rc;
  uint8_t* d = db->stage.d;
  uint8_t* h = db->stage.h;
  CmsKfdbDevQuery* hq = reinterpret_cast<CmsKfdbDevQuery*>(h + o_q);
  size_t var = o_var;
  for (int j = 0; j < njobs; ++j) {
    const cms_kfdb_job& q = jobs[j];
    CmsKfdbDevQuery& dq = hq[j];
    std::memset(&dq, 0, sizeof(dq));
    dq.mode = q.mode; dq.group = q.group; dq.min_score = q.mode == CMS_KFDB_LOOP ? q.min_score : 0.0f;
    if (q.query == CMS_KFDB_QUERY_ROW) {
      const CmsVocRow r = cms_ctx_bow_row(src, q.b, src->bow->n[(size_t)q.b]);
      dq.nwords = src->bow->nwords[(size_t)q.b]; dq.word_id = r.word_id; dq.word_val = r.word_val;
    } else if (q.query == CMS_KFDB_QUERY_SLOT) {
      dq.nwords = st->bow->nwords[(size_t)q.slot]; dq.word_id = st->bow->d_word_id + (size_t)q.slot * st->maxf; dq.word_val = st->bow->d_word_val + (size_t)q.slot * st->maxf;
    } else {
      dq.nwords = q.nwords;
      dq.word_val = (const double*)(d + var); if (q.nwords > 0) std::memcpy(h + var, q.word_val, 8 * (size_t)q.nwords); var += cms_align(8 * (size_t)q.nwords);
      dq.word_id = (const int*)(d + var); if (q.nwords > 0) std::memcpy(h + var, q.word_id, 4 * (size_t)q.nwords); var += cms_align(4 * (size_t)q.nwords);
    }
    if (q.mode == CMS_KFDB_LOOP) {
      int* hc = reinterpret_cast<int*>(h + var);
      int nc = 0;
      for (int i = 0; i < q.n_connected; ++i) if (rank[(size_t)q.connected[i]] >= 0) hc[nc++] = rank[(size_t)q.connected[i]];
      dq.n_conn = nc; dq.conn = (const int*)(d + var);
      var += cms_align(4 * (size_t)q.n_connected);
    }
  }
  std::memcpy(h + o_ent, ent.data(), E * sizeof(CmsKfdbDevEntry));
  std::memcpy(h + o_cov, covis.data(), 4 * E * CMS_KFDB_COVIS);
  std::memset(h + o_maxc, 0, 4 * Q);
  rc = db->stage.up(s, in_bytes, "cms_kfdb_detect");
  if (rc) return rc;
  CmsKfdbArgs a;
  a.Q = njobs; a.E = (int)E; a.maxf = st->maxf; a.cap = cand_cap;
  a.q = (const CmsKfdbDevQuery*)(d + o_q); a.ent = (const CmsKfdbDevEntry*)(d + o_ent); a.covis = (const int*)(d + o_cov);
  a.word_id = st->bow->d_word_id; a.word_val = st->bow->d_word_val;
  a.maxc = (int*)(d + o_maxc); a.common = (int*)(d + o_common); a.first = (int*)(d + o_first); a.score = (float*)(d + o_score); a.seen = (float*)(d + o_seen);
  a.firstpos = (int*)(d + o_fpos); a.reloc = db->d_reloc; a.cand = (int*)(d + o_cand); a.ncand = (int*)(d + o_ncand);
  const bool prof = g_kfdb_prof.on;
  if (prof) {
    for (hipEvent_t& e : g_kfdb_prof.ev) if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(g_kfdb_prof.ev[0], s));
  }
  const dim3 pairs((unsigned)((E + CMS_KFDB_WAVES - 1) / CMS_KFDB_WAVES), (unsigned)njobs);
  const size_t lds_q = 4 * (size_t)std::max(max_q, 1);      // <= 16383 x 4 B: inside the 64 KB a kernel may ask for without an attribute
  hipLaunchKernelGGL(k_kfdb_common, pairs, dim3(64 * CMS_KFDB_WAVES), lds_q, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_kfdb_score, pairs, dim3(64 * CMS_KFDB_WAVES), lds_q, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_kfdb_carry, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  size_t P = CMS_VOC_THREADS;
  while (P < E) P <<= 1;
  static bool lds_done[64] = {};
  rc = cms_lds_ceiling_once((const void*)k_kfdb_select, CMS_KFDB_MAX_ENTRIES * 8, src->device, lds_done);
  if (rc) return rc;
  hipLaunchKernelGGL(k_kfdb_select, dim3((unsigned)njobs), dim3(CMS_VOC_THREADS), P * 8, s, a);
  HIPCHK(hipGetLastError());
  if (prof) { HIPCHK(hipEventRecord(g_kfdb_prof.ev[1], s)); g_kfdb_prof.have = true; }
  rc = db->stage.back_and_wait(s, o_ncand, back_end, "cms_kfdb_detect");
  if (rc) return rc;
  const int* hn = reinterpret_cast<const int*>(h + o_ncand);
  const int* hcand = reinterpret_cast<const int*>(h + o_cand);
  bool overflow = false;
  for (size_t j = 0; j < Q; ++j) {
    n_cand[j] = hn[j];
    if (hn[j] > cand_cap) overflow = true;
    if (std::min(hn[j], cand_cap) > 0) std::memcpy(cand_slot + j * (size_t)cand_cap, hcand + j * (size_t)cand_cap, 4 * (size_t)std::min(hn[j], cand_cap));
  }
  if (diag) {
    const int* hcm = reinterpret_cast<const int*>(h + o_common);
    const float* hsc = reinterpret_cast<const float*>(h + o_score);
    for (size_t j = 0; j < Q; ++j)
      for (size_t e = 0; e < E; ++e) {
        if (diag_common) diag_common[j * K + (size_t)order[e]] = hcm[j * E + e];
        if (diag_score) diag_score[j * K + (size_t)order[e]] = hsc[j * E + e];
      }
  }
  if (overflow) return cms_fail(CMS_ERR_OVERFLOW, "cms_kfdb_detect: a query has more candidates than cand_cap (n_cand says how many)");
  return CMS_OK;
}

// mpORBVocabulary->score(CurrentBowVec, pKF->mBowVec) for pairs of slots (LoopClosing.cpp:125-138): the same ordered sum, as a double.  On the store's
// stream, synchronous.
extern "C" int cms_kfstore_bow_score(cms_kfstore* st, int npairs, const int* slot_a, const int* slot_b, double* score) {
  if (!st || npairs < 0 || (npairs > 0 && (!slot_a || !slot_b || !score))) return cms_fail(CMS_ERR_ARG, "cms_kfstore_bow_score: bad argument");
  for (int i = 0; i < npairs; ++i)
    if (!kfdb_slot_has_bow(st, slot_a[i]) || !kfdb_slot_has_bow(st, slot_b[i])) return cms_fail(CMS_ERR_ARG, "cms_kfstore_bow_score: a slot is empty or has no BowVector");
  if (npairs == 0) return CMS_OK;
  cms_ctx* c = st->c;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(kfstore_order_behind_puts(st));
  CmsStoreBow* w = st->bow;
  const size_t N = (size_t)npairs;
  CmsBlock blk;
  const size_t o_a = blk.take(4 * N), o_b = blk.take(4 * N), in_bytes = blk.size, o_s = blk.take(8 * N);
  hipStream_t s = c->stream;
  int rc = w->tmp.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  std::memcpy(w->tmp.h + o_a, slot_a, 4 * N);
  std::memcpy(w->tmp.h + o_b, slot_b, 4 * N);
  rc = w->tmp.up(s, in_bytes, "cms_kfstore_bow_score");
  if (rc) return rc;
  const CmsKfdbPairs a = {npairs, st->maxf, (const int*)(w->tmp.d + o_a), (const int*)(w->tmp.d + o_b), w->d_word_id, w->d_word_val, w->d_nwords, (double*)(w->tmp.d + o_s)};
  hipLaunchKernelGGL(k_kfdb_pair_score, dim3((unsigned)((N + CMS_KFDB_WAVES - 1) / CMS_KFDB_WAVES)), dim3(64 * CMS_KFDB_WAVES), 0, s, a);
  HIPCHK(hipGetLastError());
  rc = w->tmp.back_and_wait(s, o_s, blk.size, "cms_kfstore_bow_score");
  if (rc) return rc;
  std::memcpy(score, w->tmp.h + o_s, 8 * N);
  return CMS_OK;
}
