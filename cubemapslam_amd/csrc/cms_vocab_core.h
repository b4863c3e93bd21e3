// cms_vocab_core.h -- the numeric core of DBoW2's vocabulary-tree transform as ORBVocabulary uses it (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:
// the single-descriptor descent :1218-1259, the batch transform :1127-1194; BowVector.cpp:34-84 addWeight / addIfNotExist / normalize).  ONE source
// for the host build (libcubemapslam_host.so: hm_vocab_transform, the definition of record) and for the gfx950 kernels (cms_vocab_kernels.hip).
// It compiles under g++ as it stands.
//
// Determinism contract: the descent is integer (popcounts over 32 bytes, strict `<` so the FIRST child in `children` order wins a tie); the values
// are doubles combined with plain IEEE + / sqrt fabs in the order this source fixes (a word's value under addWeight is w added to itself count-1
// times, the L1 norm is summed over the words in ascending id order); both builds use -ffp-contract=off.  The same inputs give the same bits from
// g++ and from hipcc.
//
// The tree is walked in a re-laid form (cms_vocab_relayout): breadth first, so that the children of a node are contiguous and in `children` order
// (the file's order: ascending node id); info[node] = first child << 5 | number of children (0 = leaf).  Outputs carry the FILE's node ids and
// word ids (file_id[], word[]).
//
// Fixed where the reference is undefined (DESIGN.md "ComputeBoW"): a descent that reaches a leaf above level L - levelsup reports that leaf's node
// id as nid (the reference leaves *nid unset).
#ifndef CMS_VOCAB_CORE_H
#define CMS_VOCAB_CORE_H
#include <math.h>
#include <stdint.h>
#include "cms_detmath.h"      // CMS_HD

// DBoW2::WeightingType / ScoringType (BowVector.h:36-53)
#define CMS_VOC_TF_IDF 0
#define CMS_VOC_TF 1
#define CMS_VOC_IDF 2
#define CMS_VOC_BINARY 3
#define CMS_VOC_L1_NORM 0
#define CMS_VOC_L2_NORM 1
#define CMS_VOC_DOT_PRODUCT 5
#define CMS_VOC_MAX_K 20            // loadFromTextFile's ranges (:1359)
#define CMS_VOC_MAX_L 10
#define CMS_VOC_MAX_NODES (1 << 21)      // node ids take 21 bits of the build kernel's sort keys (ORBvoc.txt: 1 082 073 nodes)

struct CmsVocabView {
  int k, L, scoring, weighting, n_nodes, n_words;
  const uint32_t* info;            // [n_nodes] re-laid: first child << 5 | children
  const uint32_t* desc;            // [n_nodes x 8] re-laid descriptors
  const int* file_id;              // [n_nodes] re-laid node -> the file's node id
  const int* word;                 // [n_nodes] re-laid node -> word id (leaves), -1 otherwise
  const double* word_weight;       // [n_words]
};

// FORB::distance (FORB.cpp:80-101): the bit count of a ^ b over 8 words
CMS_HD int cms_vocab_distance(const uint32_t* a, const uint32_t* b) {
  int d = 0;
  for (int i = 0; i < 8; ++i) d += __builtin_popcount(a[i] ^ b[i]);
  return d;
}
// what the minimum is taken over: the smaller distance wins, then the earlier child (`d < best_d`, strict, :1244)
CMS_HD uint32_t cms_vocab_key(int dist, int child) { return ((uint32_t)dist << 8) | (uint32_t)child; }
// mustNormalize (ScoringObject.h:74-89): every scoring but DOT_PRODUCT normalises, L2_NORM with the L2 norm, the rest with L1
CMS_HD bool cms_vocab_must_normalize(int scoring, bool* l2) {
  *l2 = scoring == CMS_VOC_L2_NORM;
  return scoring != CMS_VOC_DOT_PRODUCT;
}
// a word that `count` features fell into: addWeight inserts w and then adds w count-1 times (TF, TF_IDF); addIfNotExist keeps the first w
CMS_HD double cms_vocab_word_value(int weighting, double w, int count) {
  double v = w;
  if (weighting == CMS_VOC_TF || weighting == CMS_VOC_TF_IDF)
    for (int i = 1; i < count; ++i) v += w;
  return v;
}
// one term of BowVector::normalize's sum (BowVector.cpp:67-76)
CMS_HD double cms_vocab_norm_term(bool l2, double v) { return l2 ? v * v : fabs(v); }

// transform(feature, word_id, weight, nid, levelsup) (:1218-1259); *leaf receives the re-laid index of the word's node
CMS_HD void cms_vocab_descend(const CmsVocabView& v, const uint32_t* f, int levelsup, int* word, int* nid, int* leaf) {
  const int nid_level = v.L - levelsup;
  int node = 0, level = 0, nid_out = nid_level <= 0 ? 0 : -1;
  uint32_t inf = v.info[0];
  do {
    ++level;
    const int first = (int)(inf >> 5), nc = (int)(inf & 31u);
    uint32_t best = 0xFFFFFFFFu;
    for (int c = 0; c < nc; ++c) {
      const uint32_t key = cms_vocab_key(cms_vocab_distance(f, v.desc + 8 * (size_t)(first + c)), c);
      if (key < best) best = key;
    }
    node = first + (int)(best & 0xFFu);
    if (level == nid_level) nid_out = v.file_id[node];
    inf = v.info[node];
  } while (inf & 31u);
  if (nid_out < 0) nid_out = v.file_id[node];      // a leaf above the nid level
  *word = v.word[node]; *nid = nid_out; *leaf = node;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// host only from here: the checks and the re-laying that cms_vocab_create and the host build share, and the batch transform of record
#include <map>
#include <vector>

struct CmsVocabTree {
  int k = 0, L = 0, scoring = 0, weighting = 0, n_nodes = 0, n_words = 0;
  std::vector<uint32_t> info, desc;
  std::vector<int> file_id, word;
  std::vector<double> word_weight;
  CmsVocabView view() const {
    return CmsVocabView{k, L, scoring, weighting, n_nodes, n_words, info.data(), desc.data(), file_id.data(), word.data(), word_weight.data()};
  }
};

// The tree as the text format holds it: node 0 is the root (its parent / leaf flag / descriptor / weight are not read), node i > 0 has parent[i] < i,
// children are in ascending node id (the order loadFromTextFile pushes them), word ids count the leaves in node order.  Returns NULL, or why the tree
// is refused.
inline const char* cms_vocab_relayout(int k, int L, int scoring, int weighting, int n_nodes, const int* parent, const uint8_t* is_leaf, const uint8_t* desc,
                                      const double* weight, CmsVocabTree* out) {
  if (k < 0 || k > CMS_VOC_MAX_K || L < 1 || L > CMS_VOC_MAX_L || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3)
    return "vocabulary: k, L, scoring or weighting outside the format's ranges (k 0..20, L 1..10, scoring 0..5, weighting 0..3)";
  if (n_nodes < 2) return "vocabulary: no words";
  if (n_nodes > CMS_VOC_MAX_NODES) return "vocabulary: more than 2^21 nodes";
  if (!parent || !is_leaf || !desc || !weight) return "vocabulary: null array";
  const size_t N = (size_t)n_nodes;
  std::vector<int> count(N, 0), first(N + 1, 0);
  for (size_t i = 1; i < N; ++i) {
    if (parent[i] < 0 || (size_t)parent[i] >= i) return "vocabulary: a node's parent id is not smaller than its own id";
    if (parent[i] > 0 && is_leaf[parent[i]]) return "vocabulary: a node flagged as a leaf has children";
    if (++count[(size_t)parent[i]] > k) return "vocabulary: a node has more than k children";
  }
  for (size_t i = 0; i < N; ++i)
    if (count[i] == 0 && !(i > 0 && is_leaf[i])) return "vocabulary: a node flagged as an inner node has no children";
  // children lists in file order, as CSR
  for (size_t i = 0; i < N; ++i) first[i + 1] = first[i] + count[i];
  std::vector<int> child(N > 1 ? N - 1 : 1), fill(first.begin(), first.end() - 1);
  for (size_t i = 1; i < N; ++i) child[(size_t)fill[(size_t)parent[i]]++] = (int)i;
  CmsVocabTree& t = *out;
  t.k = k; t.L = L; t.scoring = scoring; t.weighting = weighting; t.n_nodes = n_nodes;
  t.info.assign(N, 0); t.desc.assign(8 * N, 0); t.file_id.assign(N, 0); t.word.assign(N, -1);
  std::vector<int> word_of(N, -1);
  int nw = 0;
  for (size_t i = 1; i < N; ++i)
    if (is_leaf[i]) word_of[i] = nw++;
  t.n_words = nw;
  t.word_weight.assign((size_t)nw, 0.0);
  // breadth first: position p holds file node file_id[p]; its children take the next free positions
  size_t next = 1;
  for (size_t p = 0; p < N; ++p) {
    const size_t id = (size_t)t.file_id[p];
    t.info[p] = count[id] ? ((uint32_t)next << 5) | (uint32_t)count[id] : 0u;
    for (int c = 0; c < count[id]; ++c) t.file_id[next++] = child[(size_t)first[id] + (size_t)c];
    if (id > 0) {
      const uint8_t* d = desc + 32 * id;
      for (int w = 0; w < 8; ++w)
        t.desc[8 * p + (size_t)w] = (uint32_t)d[4 * w] | ((uint32_t)d[4 * w + 1] << 8) | ((uint32_t)d[4 * w + 2] << 16) | ((uint32_t)d[4 * w + 3] << 24);
    }
    t.word[p] = word_of[id];
    if (word_of[id] >= 0) t.word_weight[(size_t)word_of[id]] = weight[id];
  }
  return nullptr;
}

// transform(features, v, fv, levelsup) (:1127-1194) with BowVector::normalize (BowVector.cpp:62-84), std::map for std::map.  desc: n x 32 bytes.
// The vectors come back flattened: words ascending with their values; nodes ascending, a node's features in feature order (CSR).
struct CmsVocabResult {
  std::vector<int> word_id; std::vector<double> word_val;
  std::vector<int> node_id, node_off, node_feat;
};
inline void cms_vocab_transform_host(const CmsVocabView& v, int n, const uint8_t* desc, int levelsup, CmsVocabResult* out) {
  std::map<int, double> bow;
  std::map<int, std::vector<int>> fv;
  bool l2 = false;
  const bool must = cms_vocab_must_normalize(v.scoring, &l2);
  const bool add = v.weighting == CMS_VOC_TF || v.weighting == CMS_VOC_TF_IDF;
  for (int i = 0; i < n; ++i) {
    uint32_t f[8];
    const uint8_t* d = desc + 32 * (size_t)i;
    for (int w = 0; w < 8; ++w) f[w] = (uint32_t)d[4 * w] | ((uint32_t)d[4 * w + 1] << 8) | ((uint32_t)d[4 * w + 2] << 16) | ((uint32_t)d[4 * w + 3] << 24);
    int id, nid, leaf;
    cms_vocab_descend(v, f, levelsup, &id, &nid, &leaf);
    const double w = v.word_weight[id];
    if (w > 0) {      // not stopped
      auto it = bow.lower_bound(id);
      if (it != bow.end() && !(id < it->first)) { if (add) it->second += w; }      // addWeight / addIfNotExist
      else bow.insert(it, std::make_pair(id, w));
      fv[nid].push_back(i);
    }
  }
  if (add && !bow.empty() && !must) {
    const double nd = (double)bow.size();
    for (auto& e : bow) e.second /= nd;
  }
  if (must) {
    double norm = 0.0;
    for (auto& e : bow) norm += cms_vocab_norm_term(l2, e.second);
    if (l2) norm = sqrt(norm);
    if (norm > 0.0)
      for (auto& e : bow) e.second /= norm;
  }
  out->word_id.clear(); out->word_val.clear(); out->node_id.clear(); out->node_off.assign(1, 0); out->node_feat.clear();
  for (auto& e : bow) { out->word_id.push_back(e.first); out->word_val.push_back(e.second); }
  for (auto& e : fv) {
    out->node_id.push_back(e.first);
    out->node_feat.insert(out->node_feat.end(), e.second.begin(), e.second.end());
    out->node_off.push_back((int)out->node_feat.size());
  }
}
#endif
