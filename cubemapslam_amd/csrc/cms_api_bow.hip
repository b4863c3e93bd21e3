// cms_api_bow.hip -- host side of ORBMatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBMatcher.cpp:409-539) and of
// ORBMatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (:541-674), included by cms_lib.hip after cms_api_tri.hip (cms_kfstore).  The
// entries here and the resident (KeyFrame, Frame) ones (cms_api_vocab.hip) go through bow_run: they stage what comes from the host (FeatureVectors,
// skip flags, job records; for the stand-alone entry the key frame too) in the pinned block of the context's CmsStage (laid out with CmsBlock, 4 bytes
// of slack behind every piece), make ONE copy to the device, ONE launch of the overload's kernel and ONE copy back.
#include <algorithm>
#include <cstring>
#include <vector>

namespace {
// a FeatureVector in CSR: node ids strictly ascending, offsets ascending from >= 0, indices in [0, n); unique_of (n bytes of scratch, or NULL) also
// rejects an index listed twice -- the frame side, where DBoW2 puts every feature into exactly one node
int bow_check_fv(int n, int nnodes, const int* node_id, const int* node_off, const int* node_feat, std::vector<uint8_t>* unique_of, const char* who) {
  if (nnodes < 0 || (nnodes > 0 && (!node_id || !node_off || !node_feat)) || (nnodes > 0 && node_off[0] < 0)) return cms_fail(CMS_ERR_ARG, who);
  if (unique_of) unique_of->assign((size_t)std::max(n, 1), 0);
  for (int e = 0; e < nnodes; ++e) {
    if (e > 0 && node_id[e] <= node_id[e - 1]) return cms_fail(CMS_ERR_ARG, "SearchByBoW: FeatureVector node ids must ascend");
    if (node_off[e + 1] < node_off[e]) return cms_fail(CMS_ERR_ARG, "SearchByBoW: FeatureVector offsets must ascend");
    for (int q = node_off[e]; q < node_off[e + 1]; ++q) {
      const int f = node_feat[q];
      if (f < 0 || f >= n) return cms_fail(CMS_ERR_ARG, "SearchByBoW: FeatureVector index out of range");
      if (unique_of) {
        if ((*unique_of)[(size_t)f]) return cms_fail(CMS_ERR_ARG, "SearchByBoW: the frame's FeatureVector lists a feature twice");
        (*unique_of)[(size_t)f] = 1;
      }
    }
  }
  return CMS_OK;
}
int bow_check_frame(cms_ctx* c, int b, int n, const char* who) {
  if (b < 0 || b >= c->max_batch || n < 0) return cms_fail(CMS_ERR_ARG, who);
  if (n > CMS_AREA_MAXKP) return cms_fail(CMS_ERR_UNSUPPORTED, "SearchByBoW: more than 16383 key points in the frame");
  if (n > c->g.kp_cap) return cms_fail(CMS_ERR_ARG, "SearchByBoW: more key points than a frame row of the context holds");
  return CMS_OK;
}

// A job as the host lays it out: where each host array goes in the staged input block (offsets), and what is already on the device.
struct BowStage {
  const void* src; size_t bytes; size_t at;
};
// what bow_run needs of a job record: the entries of its index output, where the outputs go, and the overload's kernel
inline size_t bow_out_n(const CmsBowJob& q) { return (size_t)q.n; }
inline size_t bow_out_n(const CmsBowKfJob& q) { return (size_t)q.n1; }
inline void bow_set_out(CmsBowJob& q, int* idx, int* nm) { q.kf_idx = idx; q.n_matches = nm; }
inline void bow_set_out(CmsBowKfJob& q, int* idx, int* nm) { q.idx2 = idx; q.n_matches = nm; }
inline void bow_launch(const CmsBowJob* d, int njobs, hipStream_t s, float nnratio, int check_orientation) {
  hipLaunchKernelGGL(k_search_by_bow, dim3(njobs), dim3(CMS_BOW_THREADS), 0, s, d, nnratio, check_orientation);
}
inline void bow_launch(const CmsBowKfJob* d, int njobs, hipStream_t s, float nnratio, int check_orientation) {
  hipLaunchKernelGGL(k_search_by_bow_kf, dim3(njobs), dim3(CMS_BOW_THREADS), 0, s, d, nnratio, check_orientation);
}
// stage -> device -> launch -> back.  jobs[j] has every device pointer filled except the ones given as offsets in rel[j] (pointer fields that
// hold an offset into the input block, marked by the caller), which are rebased here once the block's device address is known.
template <class Job>
int bow_run(cms_ctx* c, std::vector<Job>& jobs, const std::vector<std::vector<const void**>>& rel, std::vector<BowStage>& pieces, CmsBlock blk,
            float nnratio, int check_orientation, int* out_idx, int* n_matches, const char* who) {
  const int njobs = (int)jobs.size();
  size_t total_n = 0;
  for (const Job& q : jobs) total_n += bow_out_n(q);
  const size_t o_jobs = blk.take((size_t)njobs * sizeof(Job)), o_idx = blk.take(total_n * 4, 4), o_nm = blk.take((size_t)njobs * 4);      // behind the staged pieces
  const size_t bytes = blk.size;
  hipStream_t s = c->stream;
  int rc = c->stage.reserve(s, bytes, bytes);
  if (rc) return rc;
  uint8_t* p = c->stage.d;
  uint8_t* h = c->stage.h;
  for (const BowStage& g : pieces) if (g.bytes) std::memcpy(h + g.at, g.src, g.bytes);
  size_t cursor = 0;
  for (int j = 0; j < njobs; ++j) {
    Job& q = jobs[(size_t)j];
    for (const void** f : rel[(size_t)j]) *f = p + (size_t)(uintptr_t)(*f);
    bow_set_out(q, (int*)(p + o_idx) + cursor, (int*)(p + o_nm) + j);
    cursor += bow_out_n(q);
  }
  std::memcpy(h + o_jobs, jobs.data(), (size_t)njobs * sizeof(Job));
  rc = c->stage.up(s, o_idx, who);
  if (rc) return rc;
  bow_launch((const Job*)(p + o_jobs), njobs, s, nnratio, check_orientation);
  HIPCHK(hipGetLastError());
  rc = c->stage.back_and_wait(s, o_idx, bytes, who);
  if (rc) return rc;
  if (total_n) std::memcpy(out_idx, h + o_idx, total_n * 4);
  std::memcpy(n_matches, h + o_nm, (size_t)njobs * 4);
  return CMS_OK;
}
// host array -> staged piece; the job field receives its offset in the block (rebased by bow_run)
template <class T>
void bow_put(std::vector<BowStage>& pieces, CmsBlock& blk, std::vector<const void**>& rel, const T*& field, const void* src, size_t bytes) {
  const size_t at = blk.take(bytes, 4);
  pieces.push_back(BowStage{src, bytes, at});
  field = reinterpret_cast<const T*>((uintptr_t)at);
  rel.push_back(reinterpret_cast<const void**>(&field));
}
}  // namespace

// Tracking::TrackReferenceKeyFrame's matcher (Tracking.cpp:567-618) with the key frame from the host: frame b of ctx's last batch against kf
extern "C" int cms_search_by_bow(cms_ctx* c, int b, int n, int nnodes, const int* node_id, const int* node_off, const int* node_feat, const cms_keyframe* kf,
                                 const uint8_t* kf_skip, float nnratio, int check_orientation, int* kf_idx, int* n_matches) {
  if (!c || !kf || !n_matches || (n > 0 && !kf_idx)) return cms_fail(CMS_ERR_ARG, "cms_search_by_bow: bad argument");
  int rc = bow_check_frame(c, b, n, "cms_search_by_bow: bad frame");
  if (rc) return rc;
  if (kf->n > CMS_TRI_MAXF) return cms_fail(CMS_ERR_UNSUPPORTED, "cms_search_by_bow: more than 4096 features in the key frame");
  if (kf->n < 0 || (kf->n > 0 && (!kf->kps || !kf->desc || !kf->mp))) return cms_fail(CMS_ERR_ARG, "cms_search_by_bow: bad key frame");
  std::vector<uint8_t> seen;
  rc = bow_check_fv(kf->n, kf->nnodes, kf->node_id, kf->node_off, kf->node_feat, nullptr, "cms_search_by_bow: bad key-frame FeatureVector");
  if (rc) return rc;
  rc = bow_check_fv(n, nnodes, node_id, node_off, node_feat, &seen, "cms_search_by_bow: bad frame FeatureVector");
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  std::vector<CmsBowJob> jobs(1);
  std::vector<std::vector<const void**>> rel(1);
  std::vector<BowStage> pieces;
  CmsBowJob& q = jobs[0];
  std::memset(&q, 0, sizeof(q));
  CmsBlock blk;
  const size_t kn = (size_t)kf->n;
  const int kfeat = kf->nnodes > 0 ? kf->node_off[kf->nnodes] : 0, ffeat = nnodes > 0 ? node_off[nnodes] : 0;
  bow_put(pieces, blk, rel[0], q.kf_kp, kf->kps, kn * sizeof(CmsKeyPoint));
  bow_put(pieces, blk, rel[0], q.kf_desc, kf->desc, kn * 32);
  bow_put(pieces, blk, rel[0], q.kf_mp, kf->mp, kn * 4);
  if (kf_skip) bow_put(pieces, blk, rel[0], q.kf_skip, kf_skip, kn);
  bow_put(pieces, blk, rel[0], q.kf_nid, kf->node_id, 4 * (size_t)kf->nnodes);
  bow_put(pieces, blk, rel[0], q.kf_noff, kf->node_off, kf->nnodes > 0 ? 4 * ((size_t)kf->nnodes + 1) : 0);
  bow_put(pieces, blk, rel[0], q.kf_nfeat, kf->node_feat, 4 * (size_t)kfeat);
  bow_put(pieces, blk, rel[0], q.f_nid, node_id, 4 * (size_t)nnodes);
  bow_put(pieces, blk, rel[0], q.f_noff, node_off, nnodes > 0 ? 4 * ((size_t)nnodes + 1) : 0);
  bow_put(pieces, blk, rel[0], q.f_nfeat, node_feat, 4 * (size_t)ffeat);
  q.kf_nnodes = kf->nnodes; q.f_nnodes = nnodes; q.n = n;
  const size_t sb = (size_t)b * c->g.kp_cap;
  q.f_kp = (const CmsKeyPoint*)c->d_kps + sb; q.f_desc = (const uint4*)(c->d_desc + 32 * sb);
  return bow_run(c, jobs, rel, pieces, blk, nnratio, check_orientation, kf_idx, n_matches, "cms_search_by_bow");
}

// LoopClosing::ComputeSim3's matcher (LoopClosing.cpp:251-279: ORBMatcher(0.75, true).SearchByBoW(mpCurrentKF, pKF, vvpMapPointMatches[i]), src/ORBMatcher.cpp:541-674)
// on resident key frames: all candidates of a pass -- of several maps or streams, if the host serves several -- in ONE launch on src's stream.
// Nothing is enqueued on the store's stream; the copies of cms_kfstore_put_from_frame(s) that filled a named slot are waited for on the device.
extern "C" int cms_kfstore_search_by_bow_keyframes(cms_kfstore* st, cms_ctx* src, int njobs, const cms_bow_kf_job* jobs, float nnratio, int check_orientation,
                                                   int* idx2, int* n_matches) {
  if (!st || !src || njobs < 0 || (njobs > 0 && (!jobs || !n_matches))) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_bow_keyframes: bad argument");
  if (njobs == 0) return CMS_OK;
  if (src->device != st->c->device) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_bow_keyframes: the context and the store must share the device");
  size_t total_n1 = 0;
  for (int j = 0; j < njobs; ++j) {
    const cms_bow_kf_job& q = jobs[j];
    const int slots[2] = {q.slot1, q.slot2}, counts[2] = {q.n1, q.n2};
    for (int k = 0; k < 2; ++k) {
      if (slots[k] < 0 || slots[k] >= st->maxkf) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_bow_keyframes: slot out of range");
      if (!st->used[(size_t)slots[k]]) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_bow_keyframes: empty slot");
      if (counts[k] != st->h_kf[(size_t)slots[k]].n) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_bow_keyframes: n1 / n2 is not the slot's stored key-point count");
    }
    total_n1 += (size_t)q.n1;
  }
  if (total_n1 > 0 && !idx2) return cms_fail(CMS_ERR_ARG, "cms_kfstore_search_by_bow_keyframes: bad argument");
  HIPCHK(hipSetDevice(src->device));
  int rc = kfstore_wait_puts(st, src->stream, 2 * njobs, [&](int j) { return (j & 1) ? jobs[j >> 1].slot2 : jobs[j >> 1].slot1; });
  if (rc) return rc;
  std::vector<CmsBowKfJob> dj((size_t)njobs);
  std::vector<std::vector<const void**>> rel((size_t)njobs);
  std::vector<BowStage> pieces;
  CmsBlock blk;
  for (int j = 0; j < njobs; ++j) {
    const cms_bow_kf_job& q = jobs[j];
    const CmsTriKF& k1 = st->h_kf[(size_t)q.slot1];
    const CmsTriKF& k2 = st->h_kf[(size_t)q.slot2];
    CmsBowKfJob& d = dj[(size_t)j];
    std::memset(&d, 0, sizeof(d));
    d.kp1 = st->d_kp + k1.f0; d.desc1 = (const uint4*)(st->d_desc + 32 * (size_t)k1.f0); d.mp1 = st->d_mp + k1.f0; d.fn1 = st->d_fn + k1.f0;
    d.nid1 = st->d_nid + k1.node0; d.noff1 = st->d_noff + k1.noff0; d.nfeat1 = st->d_nfeat + k1.nfeat0; d.n1 = k1.n; d.nnodes1 = k1.nnodes;
    d.kp2 = st->d_kp + k2.f0; d.desc2 = (const uint4*)(st->d_desc + 32 * (size_t)k2.f0); d.mp2 = st->d_mp + k2.f0; d.fn2 = st->d_fn + k2.f0;
    d.nid2 = st->d_nid + k2.node0; d.noff2 = st->d_noff + k2.noff0; d.nfeat2 = st->d_nfeat + k2.nfeat0; d.n2 = k2.n; d.nnodes2 = k2.nnodes;
    if (q.skip1) bow_put(pieces, blk, rel[(size_t)j], d.skip1, q.skip1, (size_t)k1.n);
    if (q.skip2) bow_put(pieces, blk, rel[(size_t)j], d.skip2, q.skip2, (size_t)k2.n);
  }
  return bow_run(src, dj, rel, pieces, blk, nnratio, check_orientation, idx2, n_matches, "cms_kfstore_search_by_bow_keyframes");
}
