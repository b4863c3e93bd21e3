// cms_kfdb_core.h -- the numeric core of KeyFrameDatabase::DetectRelocalizationCandidates / DetectLoopCandidates (src/KeyFrameDatabase.cpp:81-314)
// and of the L1 score they call (DBoW2 ScoringObject.cpp:23-68), on plain arrays.  ONE source for the host build (libcubemapslam_host.so: hm_kfdb_*,
// the definition of record) and for the gfx950 kernels (cms_kfdb_kernels.hip).  It compiles under g++ as it stands.
//
// A database entry is a key-frame slot with a group (one per map / camera stream: a query sees the entries of its own group only), an add sequence
// number, a persistent reloc_score (KeyFrame::mRelocScore) and up to CMS_KFDB_COVIS covisible slots, best first, padded with -1
// (GetBestCovisibilityKeyFrames(10)).
//
// Order contract: lKFsSharingWords holds the entries of the query's group that share a word with the query.  The reference meets them while it
// walks the query's words ascending and each word's inverted list in add() order, so the list is ordered by (smallest common word id, add sequence
// number); erase + add gives a new, larger number.  Everything returned is a subsequence of that order (cms_kfdb_list_key).
//
// Determinism contract: the counts are integers; minCommonWords is ONE int -> float conversion, ONE float multiply and ONE float -> int conversion;
// the score is a double sum over the common words in ascending word order of terms made of three fabs and two subtractions, then one negation, one
// division by 2.0 and one conversion to float; the accumulation over the covisibles is a float add per covisible in stored order.  Both builds use
// -ffp-contract=off.  The same inputs give the same bits from g++ and from hipcc.
//
// Fixed where the reference is undefined (DESIGN.md "KeyFrameDatabase"): a covisible that shares a word with a relocalisation query but was never
// scored by any query contributes the uninitialised KeyFrame::mRelocScore there; here reloc_score is 0.0f from add on.
#ifndef CMS_KFDB_CORE_H
#define CMS_KFDB_CORE_H
#include <math.h>
#include <stdint.h>
#include "cms_detmath.h"      // CMS_HD

#define CMS_KFDB_RELOC 0            // DetectRelocalizationCandidates (:204-314)
#define CMS_KFDB_LOOP 1             // DetectLoopCandidates (:81-202)
#define CMS_KFDB_COVIS 10           // GetBestCovisibilityKeyFrames(10) (:156, :270)
#define CMS_KFDB_NOKEY 0xFFFFFFFFFFFFFFFFull

// int minCommonWords = maxCommonWords*0.8f (:125, :240)
CMS_HD int cms_kfdb_min_common(int max_common) { return (int)((float)max_common * 0.8f); }
// one term of L1Scoring::score's sum (ScoringObject.cpp:36), vi from the query
CMS_HD double cms_kfdb_l1_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }
// score = -score/2.0 (ScoringObject.cpp:63); the callers' `float si = mpVoc->score(...)` is cms_kfdb_score_float of it
CMS_HD double cms_kfdb_l1_finish(double sum) { return -sum / 2.0; }
CMS_HD float cms_kfdb_score_float(double score) { return (float)score; }
// what lKFsSharingWords is ordered by: the smallest common word, then the rank of the entry's add sequence number among the database's entries
CMS_HD unsigned long long cms_kfdb_list_key(int first_word, int rank) { return ((unsigned long long)(unsigned)first_word << 32) | (unsigned)rank; }
// float minScoreToRetain = 0.75f*bestAccScore (:181, :295)
CMS_HD float cms_kfdb_retain(float best_acc) { return 0.75f * best_acc; }
// the first index i in ids[0, n) with ids[i] >= id (the vectors ascend strictly)
CMS_HD int cms_kfdb_lower_bound(const int* ids, int n, int id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < id) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// host only from here: the database of record
#include <algorithm>
#include <vector>

struct CmsKfdbBow { int n; const int* id; const double* val; };

// ids strictly ascending and not negative
inline bool cms_kfdb_bow_ok(int n, const int* id) {
  for (int i = 0; i < n; ++i)
    if (id[i] < 0 || (i > 0 && id[i] <= id[i - 1])) return false;
  return true;
}
// common words, the smallest of them (-1: none) and the ordered sum of the terms, v1 = a
inline void cms_kfdb_intersect_host(const CmsKfdbBow& a, const CmsKfdbBow& b, int* common, int* first, double* sum) {
  int i = 0, j = 0, c = 0, f = -1;
  double s = 0;
  while (i < a.n && j < b.n) {
    if (a.id[i] == b.id[j]) {
      if (c++ == 0) f = a.id[i];
      s += cms_kfdb_l1_term(a.val[i], b.val[j]);
      ++i; ++j;
    } else if (a.id[i] < b.id[j]) ++i;
    else ++j;
  }
  *common = c; *first = f; *sum = s;
}
inline double cms_kfdb_score_host(const CmsKfdbBow& a, const CmsKfdbBow& b) {
  int c, f;
  double s;
  cms_kfdb_intersect_host(a, b, &c, &f, &s);
  return cms_kfdb_l1_finish(s);
}

struct CmsKfdbQuery {
  int mode, group;
  CmsKfdbBow bow;
  float min_score;                        // LOOP
  int n_connected; const int* connected;  // LOOP: slots of pKF->GetConnectedKeyFrames()
};

struct CmsKfdbHost {
  struct Slot {
    bool has_bow = false, in_db = false;
    int group = 0;
    unsigned long long seq = 0;
    float reloc_score = 0.0f;
    int covis[CMS_KFDB_COVIS];
    std::vector<int> id; std::vector<double> val;
    Slot() { std::fill(covis, covis + CMS_KFDB_COVIS, -1); }
  };
  std::vector<Slot> slots;
  int max_features = 0;
  unsigned long long next_seq = 0;

  CmsKfdbHost(int max_keyframes, int max_feat) : slots((size_t)max_keyframes), max_features(max_feat) {}
  bool slot_ok(int s) const { return s >= 0 && (size_t)s < slots.size(); }
  CmsKfdbBow bow(int s) const { const Slot& e = slots[(size_t)s]; return CmsKfdbBow{(int)e.id.size(), e.id.data(), e.val.data()}; }
  // each returns 0, or -1 (the library's CMS_ERR_ARG) with nothing changed
  int set_bow(int s, int n, const int* id, const double* val) {
    if (!slot_ok(s) || n < 0 || n > max_features || (n > 0 && (!id || !val)) || !cms_kfdb_bow_ok(n, id)) return -1;
    Slot& e = slots[(size_t)s];
    e.id.assign(id, id + n); e.val.assign(val, val + n); e.has_bow = true;
    return 0;
  }
  // cms_kfstore_put*: another key frame takes the slot
  void refill(int s) { Slot& e = slots[(size_t)s]; e.has_bow = false; e.in_db = false; e.id.clear(); e.val.clear(); std::fill(e.covis, e.covis + CMS_KFDB_COVIS, -1); }
  int add(int n, const int* s, const int* groups) {
    for (int i = 0; i < n; ++i) {
      if (!slot_ok(s[i]) || !slots[(size_t)s[i]].has_bow || slots[(size_t)s[i]].in_db || groups[i] < 0) return -1;
      for (int j = 0; j < i; ++j) if (s[j] == s[i]) return -1;
    }
    for (int i = 0; i < n; ++i) {
      Slot& e = slots[(size_t)s[i]];
      e.in_db = true; e.group = groups[i]; e.seq = next_seq++; e.reloc_score = 0.0f;
    }
    return 0;
  }
  int erase(int n, const int* s) {
    for (int i = 0; i < n; ++i) if (!slot_ok(s[i])) return -1;
    for (int i = 0; i < n; ++i) slots[(size_t)s[i]].in_db = false;
    return 0;
  }
  void clear(int group) { for (Slot& e : slots) if (group < 0 || e.group == group) e.in_db = false; }
  int set_covisibles(int n, const int* s, const int* neigh) {
    for (int i = 0; i < n; ++i) {
      if (!slot_ok(s[i])) return -1;
      for (int c = 0; c < CMS_KFDB_COVIS; ++c) if (neigh[i * CMS_KFDB_COVIS + c] < -1 || neigh[i * CMS_KFDB_COVIS + c] >= (int)slots.size()) return -1;
    }
    for (int i = 0; i < n; ++i) std::copy(neigh + i * CMS_KFDB_COVIS, neigh + (i + 1) * CMS_KFDB_COVIS, slots[(size_t)s[i]].covis);
    return 0;
  }

  // One query.  cand receives the candidate slots in list order; diag_common / diag_score (NULL, or one per slot) the common words per slot and the
  // float score, -1 where the slot was not scored.
  void detect(const CmsKfdbQuery& q, std::vector<int>* cand, int* diag_common, float* diag_score) {
    const size_t K = slots.size();
    const bool loop = q.mode == CMS_KFDB_LOOP;
    std::vector<int> common(K, 0), first(K, -1);
    std::vector<double> sum(K, 0.0);
    std::vector<uint8_t> connected(K, 0);
    if (loop) for (int i = 0; i < q.n_connected; ++i) if (slot_ok(q.connected[i])) connected[(size_t)q.connected[i]] = 1;
    // ranks of the add sequence numbers
    std::vector<int> by_seq;
    for (size_t s = 0; s < K; ++s) if (slots[s].in_db) by_seq.push_back((int)s);
    std::sort(by_seq.begin(), by_seq.end(), [&](int a, int b) { return slots[(size_t)a].seq < slots[(size_t)b].seq; });
    std::vector<unsigned long long> list;
    int max_common = 0;
    for (size_t r = 0; r < by_seq.size(); ++r) {
      const size_t s = (size_t)by_seq[r];
      if (slots[s].group != q.group || connected[s]) continue;
      cms_kfdb_intersect_host(q.bow, bow((int)s), &common[s], &first[s], &sum[s]);
      if (common[s] == 0) continue;
      list.push_back(cms_kfdb_list_key(first[s], (int)r));
      max_common = std::max(max_common, common[s]);
    }
    std::sort(list.begin(), list.end());
    const int min_common = cms_kfdb_min_common(max_common);
    std::vector<float> score(K, -1.0f);
    std::vector<uint8_t> scored(K, 0);
    for (unsigned long long key : list) {
      const size_t s = (size_t)by_seq[(size_t)(key & 0xFFFFFFFFu)];
      if (common[s] > min_common) {
        scored[s] = 1; score[s] = cms_kfdb_score_float(cms_kfdb_l1_finish(sum[s]));
        if (!loop) slots[s].reloc_score = score[s];
      }
    }
    if (diag_common) std::copy(common.begin(), common.end(), diag_common);
    if (diag_score) std::copy(score.begin(), score.end(), diag_score);
    std::vector<float> acc;
    std::vector<int> best;
    float best_acc = loop ? q.min_score : 0.0f;
    for (unsigned long long key : list) {
      const size_t s = (size_t)by_seq[(size_t)(key & 0xFFFFFFFFu)];
      if (!scored[s] || (loop && !(score[s] >= q.min_score))) continue;
      float a = score[s], b = score[s];
      int who = (int)s;
      for (int c = 0; c < CMS_KFDB_COVIS; ++c) {
        const int n = slots[s].covis[c];
        if (n < 0 || common[(size_t)n] == 0) continue;      // (common is 0 for a slot outside the database, the group or, LOOP, the list)
        if (loop && !scored[(size_t)n]) continue;
        const float v = loop ? score[(size_t)n] : slots[(size_t)n].reloc_score;
        a += v;
        if (v > b) { who = n; b = v; }
      }
      acc.push_back(a); best.push_back(who);
      if (a > best_acc) best_acc = a;
    }
    const float retain = cms_kfdb_retain(best_acc);
    std::vector<uint8_t> taken(K, 0);
    cand->clear();
    for (size_t i = 0; i < acc.size(); ++i)
      if (acc[i] > retain && !taken[(size_t)best[i]]) { taken[(size_t)best[i]] = 1; cand->push_back(best[i]); }
  }
};
#endif
